"""Hand-built cost volumes for the 3-D cost-to-go field (tests/test_nav_field3d_cpu.py, tests/test_nav_field3d_gpu.py).  Every scene is (cost u8
[D, H, W], goals [S, 3 or 4], ...).  LETHAL marks a wall under the default `lethal` of 253.  TK, TI, TJ are the tile edges of tsl_nav_field3.hip along
the layer, the row and the column; every volume holds at most 40 000 cells."""
import numpy as np

LETHAL = 254
TK, TI, TJ = 8, 8, 16
# each of D, H, W once at 1, once at exactly one tile edge, once at an edge plus one cell and once at two edges plus a part
SHAPES = [(1, 1, 1), (1, TI + 1, 2 * TJ + 3), (TK + 1, TI, TJ), (2 * TK + 3, TI + 1, 1), (TK, 2 * TI + 3, TJ + 1)]
_D2 = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
_DIRS = tuple((0,) + d for d in _D2) + ((1, 0, 0),) + tuple((1,) + d for d in _D2) + ((-1, 0, 0),) + tuple((-1,) + d for d in _D2)


def components(trav, connectivity=26):
    """int32 labels [D, H, W] (0 = not traversable) of the sets of traversable cells joined by allowed moves, and the label of the largest (plain flood
    fill with the corner rule of the field: every cell of the square or cube a diagonal move spans must be traversable)"""
    D, H, W = trav.shape
    t = trav.tolist()
    label = np.zeros((D, H, W), np.int32)
    lab = label.tolist()
    nzmax = {6: 1, 18: 2, 26: 3}[connectivity]
    dirs = [d for d in _DIRS if sum(1 for v in d if v) <= nzmax]
    best, best_n, n_lab = 0, 0, 0

    def free(k, r, c):
        return 0 <= k < D and 0 <= r < H and 0 <= c < W and t[k][r][c]

    for k0, r0, c0 in np.argwhere(trav).tolist():
        if lab[k0][r0][c0]:
            continue
        n_lab += 1
        lab[k0][r0][c0] = n_lab
        stack, n = [(k0, r0, c0)], 0
        while stack:
            k, r, c = stack.pop()
            n += 1
            for dk, di, dj in dirs:
                a, b, e = k + dk, r + di, c + dj
                if not free(a, b, e) or lab[a][b][e]:
                    continue
                if not all(free(k + x * dk, r + y * di, c + z * dj) for x in (0, 1) for y in (0, 1) for z in (0, 1)):
                    continue
                lab[a][b][e] = n_lab
                stack.append((a, b, e))
        if n > best_n:
            best, best_n = n_lab, n
    return np.array(lab, np.int32).reshape(D, H, W), best


def largest_component(trav, connectivity=26):
    label, best = components(trav, connectivity)
    return label == best if best else np.zeros(trav.shape, bool)


def random_volume(D, H, W, seed=7, walls=0.35):
    """costs 0 .. 199 with about 35 % of the cells lethal; the goal is the first cell of the largest component"""
    rng = np.random.default_rng(seed + 100000 * D + 1000 * H + W)
    cost = rng.integers(0, 200, (D, H, W)).astype(np.uint8)
    cost[rng.random((D, H, W)) < walls] = LETHAL
    comp = largest_component(cost < 253)
    if not comp.any():                                            # (the 1 x 1 x 1 volume may be a wall: open it)
        cost[0, 0, 0] = 0
        comp = largest_component(cost < 253)
    k, r, c = np.argwhere(comp)[0].tolist()
    return cost, np.array([[k, r, c]], np.int32), comp


def binary_volume(connectivity=26, D=11, H=19, W=21):
    """costs 0 and 1, three cells in ten 1: with lethal = 1 only cost 0 is traversable; the goal is in the largest component"""
    rng = np.random.default_rng(21)
    cost = (rng.random((D, H, W)) < 0.3).astype(np.uint8)
    comp = largest_component(cost < 1, connectivity)
    k, r, c = np.argwhere(comp)[0].tolist()
    return cost, np.array([[k, r, c]], np.int32), comp


def serpentine(n=24, kp=4, ip=4):
    """slabs of kp - 1 free layers between wall layers with one hole each, at alternating corners, and inside each slab a snake: walls every `ip` rows
    through all of the slab's layers, open for one column at alternating ends.  The way from (0, 0, 0) crosses every slab from corner to corner."""
    cost = np.zeros((n, n, n), np.uint8)
    for m, r in enumerate(range(ip - 1, n - 1, ip)):
        cost[:, r, :] = LETHAL
        if m % 2 == 0:
            cost[:, r, n - 1] = 0
        else:
            cost[:, r, 0] = 0
    n_walls = len(range(ip - 1, n - 1, ip))
    far = (n - 1, n - 1) if n_walls % 2 else (n - 1, 0)        # where the snake that starts at (0, 0) ends
    for m, k in enumerate(range(kp - 1, n - 1, kp)):
        cost[k] = LETHAL
        if m % 2 == 0:
            cost[k, far[0], far[1]] = 0
        else:
            cost[k, 0, 0] = 0
    return cost, np.array([[0, 0, 0]], np.int32)


def face_diagonal(walled):
    """a 4 x 4 x 4 block of walls with the square (1, 1 .. 2, 1 .. 2) free but for cell `walled` of its two off-diagonal cells (None: all four free);
    the goal is (1, 1, 1), the cell across the diagonal (1, 2, 2)"""
    cost = np.full((4, 4, 4), LETHAL, np.uint8)
    cost[1, 1:3, 1:3] = 0
    if walled is not None:
        cost[(1,) + ((1, 2), (2, 1))[walled]] = LETHAL
    return cost, np.array([[1, 1, 1]], np.int32)


SPACE_CELLS = ((1, 1, 2), (1, 2, 1), (2, 1, 1), (1, 2, 2), (2, 1, 2), (2, 2, 1))       # the six other cells of the cube between (1, 1, 1) and (2, 2, 2)


def space_diagonal(walled):
    """a 4 x 4 x 4 block of walls with the cube (1 .. 2)^3 free but for cell SPACE_CELLS[walled] (None: all eight free); the goal is (1, 1, 1), the cell
    across the space diagonal (2, 2, 2)"""
    cost = np.full((4, 4, 4), LETHAL, np.uint8)
    cost[1:3, 1:3, 1:3] = 0
    if walled is not None:
        cost[SPACE_CELLS[walled]] = LETHAL
    return cost, np.array([[1, 1, 1]], np.int32)


UNIFORM_SEED = (8, 9, 17)


def uniform(D=17, H=19, W=35, c=0):
    """one central seed in a uniform volume: every parent is hand-worked from the <5, 7, 9> chamfer distance"""
    return np.full((D, H, W), c, np.uint8), np.array([list(UNIFORM_SEED)], np.int32)


def uniform_two_seeds(D=17, H=19, W=35):
    """two seeds above one another: the cells half way tie between a move up and a move down (one seed in a uniform volume cannot produce that tie)"""
    return np.full((D, H, W), 0, np.uint8), np.array([[4, 9, 17], [12, 9, 17]], np.int32)


def checkerboard(D=9, H=17, W=19, a=10, b=60):
    k, i, j = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return np.where((k + i + j) & 1, a, b).astype(np.uint8), np.array([[7, 13, 3]], np.int32)


def many_seeds():
    """seeds with unequal values, one dominated by its neighbour, duplicates on one cell, seeds on a tile face, a tile edge and a tile corner, and bad
    ones: on a wall and outside on each of the six sides"""
    rng = np.random.default_rng(11)
    cost = rng.integers(0, 120, (20, 20, 40)).astype(np.uint8)
    cost[10, 2:18, 3:36] = LETHAL
    goals = np.array([[1, 3, 3, 0], [18, 17, 36, 1000], [3, 10, 30, 250],
                      [3, 10, 31, 250 + 9000],                    # dominated: its neighbour (3, 10, 30) reaches it for far less
                      [15, 12, 22, 900], [15, 12, 22, 700], [15, 12, 22, 800],      # duplicates: 700 counts
                      [TK, 3, 5, 300], [TK - 1, TI, 5, 310], [TK, TI, TJ, 320], [2 * TK - 1, 2 * TI - 1, 2 * TJ - 1, 330],      # tile face, edge, corners
                      [10, 10, 20, 0],                            # on the wall
                      [-1, 3, 3, 0], [20, 3, 3, 0], [3, -1, 3, 0], [3, 20, 3, 0], [3, 3, -1, 0], [3, 3, 40, 0]], np.int32)      # outside, each side
    return cost, goals, 7                                          # the number of bad seeds


def saturated():
    """a seed value 100 below 2^32: every other cell clips to 2^32 - 2"""
    return np.zeros((2, 3, 40), np.uint8), np.array([[0, 0, 0, -100]], np.int64)


def walled_in():
    """a free room with a sealed cell inside it: (5, 5, 5) is traversable and reaches nothing"""
    cost = np.zeros((10, 12, 20), np.uint8)
    cost[4:7, 4:7, 4:7] = LETHAL
    cost[5, 5, 5] = 0
    return cost, np.array([[8, 10, 15]], np.int32)
