"""Term lists that exercise the sum of products' bookkeeping, shared by tests/test_gpu_sop.py (the device), tests/test_oracle_sop_c.py
(the C oracle) and tests/test_gpu_sop_sizes.py: name -> (number of tables, terms)."""

from oracle.field import P

BOOKKEEPING = {
    "mixed degrees under D = 3": (3, [(1, (0, 1, 2)), (3, (1, 2)), (P - 5, (0,))]),
    "square, cube, a table in three terms": (2, [(1, (0, 0)), (2, (0, 0, 0)), (3, (0, 1)), (4, (1,))]),
    "cube alone": (1, [(7, (0, 0, 0))]),
    "eight terms over eight tables": (8, [((0, 1, P - 1, 0x1234567890ABCDEF << 180, 2, P - 2, 1, 5)[k], (k, (k + 1) % 8, (k + 3) % 8)[:1 + k % 3])
                                          for k in range(8)]),
    "zero and one and r - 1": (3, [(0, (0, 1)), (1, (1, 2)), (P - 1, (0,))]),
}
