"""Hand-built cost planes for the cost-to-go field (tests/test_nav_field_cpu.py, tests/test_nav_field_gpu.py).  Every scene is (cost u8 [H, W] or
[B, H, W], goals [S, 3 or 4], keywords of the call).  LETHAL marks a wall under the default `lethal` of 253."""
import numpy as np

LETHAL = 254
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 31), (65, 97)]          # partial tiles, a tile edge plus one cell


def largest_component(trav, connectivity=8):
    """bool mask of the largest set of traversable cells joined by allowed moves (plain flood fill; the corner rule of the field)"""
    H, W = trav.shape
    label = np.zeros((H, W), np.int32)
    best, best_n, n_lab = 0, 0, 0
    dirs = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
    for r0, c0 in np.argwhere(trav).tolist():
        if label[r0, c0]:
            continue
        n_lab += 1
        label[r0, c0] = n_lab
        stack, n = [(r0, c0)], 0
        while stack:
            r, c = stack.pop()
            n += 1
            for d, (di, dj) in enumerate(dirs):
                if (d & 1) and connectivity != 8:
                    continue
                a, b = r + di, c + dj
                if not (0 <= a < H and 0 <= b < W) or not trav[a, b] or label[a, b]:
                    continue
                if (d & 1) and not (trav[r + di, c] and trav[r, c + dj]):
                    continue
                label[a, b] = n_lab
                stack.append((a, b))
        if n > best_n:
            best, best_n = n_lab, n
    return label == best if best else np.zeros((H, W), bool)


def random_plane(H, W, seed=7):
    """costs 0 .. 199 with a quarter of the cells lethal; the goal is the first cell of the largest component"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    cost = rng.integers(0, 200, (H, W)).astype(np.uint8)
    cost[rng.random((H, W)) < 0.25] = LETHAL
    comp = largest_component(cost < 253)
    if not comp.any():                                            # (the 1 x 1 plane may be a wall: open it)
        cost[0, 0] = 0
        comp = largest_component(cost < 253)
    r, c = np.argwhere(comp)[0].tolist()
    return cost, np.array([[0, r, c]], np.int32), comp


def binary_plane(connectivity=8, H=40, W=45):
    """costs 0 and 1, three cells in ten 1: with lethal = 1 only cost 0 is traversable; the goal is in the largest component"""
    rng = np.random.default_rng(21)
    cost = (rng.random((H, W)) < 0.3).astype(np.uint8)
    comp = largest_component(cost < 1, connectivity)
    r, c = np.argwhere(comp)[0].tolist()
    return cost, np.array([[0, r, c]], np.int32), comp


def serpentine(n=96, pitch=8, gap=3):
    """walls every `pitch` rows with `gap`-cell openings at alternating ends: the way from the first row to the last crosses the plane once per wall"""
    cost = np.zeros((n, n), np.uint8)
    for k, r in enumerate(range(pitch - 1, n - 1, pitch)):
        cost[r, :] = LETHAL
        if k % 2 == 0:
            cost[r, n - gap:] = 0
        else:
            cost[r, :gap] = 0
    return cost, np.array([[0, 0, 0]], np.int32)


def corner_block():
    """a 2 x 2 block [[0, L], [L, 0]] walled into a 5 x 5 plane: the two free cells touch only at a corner"""
    cost = np.full((5, 5), LETHAL, np.uint8)
    cost[1, 1] = cost[2, 2] = 0
    return cost, np.array([[0, 1, 1]], np.int32)


def diagonal_corridor(n=12):
    """a 1-wide diagonal corridor: every step of it would cut a corner"""
    cost = np.full((n, n), LETHAL, np.uint8)
    for k in range(n):
        cost[k, k] = 0
    return cost, np.array([[0, 0, 0]], np.int32)


def staircase_corridor(n=12):
    """the same corridor made 4-connected: (k, k) and (k, k + 1)"""
    cost = np.full((n, n), LETHAL, np.uint8)
    for k in range(n):
        cost[k, k] = 0
        if k + 1 < n:
            cost[k, k + 1] = 0
    return cost, np.array([[0, 0, 0]], np.int32)


def uniform(H=40, W=45, c=0):
    return np.full((H, W), c, np.uint8), np.array([[0, 17, 20]], np.int32)


def checkerboard(H=40, W=45, a=10, b=60):
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.where((i + j) & 1, a, b).astype(np.uint8), np.array([[0, 33, 3]], np.int32)


def many_seeds():
    """several seeds with unequal values, one dominated by its neighbour, duplicates on one cell, and bad ones: on a wall, outside, in a wrong plane"""
    rng = np.random.default_rng(11)
    cost = rng.integers(0, 120, (50, 70)).astype(np.uint8)
    cost[20, 5:60] = LETHAL
    goals = np.array([[0, 3, 3, 0], [0, 45, 60, 1000], [0, 10, 40, 250],
                      [0, 10, 41, 250 + 5000],                    # dominated: its neighbour (10, 40) reaches it for far less
                      [0, 30, 30, 900], [0, 30, 30, 700], [0, 30, 30, 800],      # duplicates: 700 counts
                      [0, 20, 30, 0],                             # on the wall
                      [0, -1, 5, 0], [0, 50, 0, 0], [0, 5, 70, 0], [1, 3, 3, 0], [-1, 3, 3, 0]], np.int32)      # outside, wrong plane
    return cost, goals, 6                                          # the number of bad seeds


def sixteen_planes(H=45, W=50):
    rng = np.random.default_rng(5)
    cost = rng.integers(0, 200, (16, H, W)).astype(np.uint8)
    cost[rng.random((16, H, W)) < 0.2] = LETHAL
    goals = []
    for b in range(16):
        comp = largest_component(cost[b] < 253)
        r, c = np.argwhere(comp)[b % int(comp.sum())].tolist()
        goals.append([b, r, c, 10 * b])
    return cost, np.array(goals, np.int32)


def ribbon(W=4096):
    """3 x W, the widest plane there is: random costs with walls in the outer rows only, the goal at one end"""
    rng = np.random.default_rng(9)
    cost = rng.integers(0, 200, (3, W)).astype(np.uint8)
    cost[0, rng.random(W) < 0.3] = LETHAL
    cost[2, rng.random(W) < 0.3] = LETHAL
    return cost, np.array([[0, 1, 0]], np.int32)


def walled_in():
    """a free room with a sealed cell inside it: (5, 5) is traversable and reaches nothing"""
    cost = np.zeros((20, 20), np.uint8)
    cost[4:7, 4:7] = LETHAL
    cost[5, 5] = 0
    return cost, np.array([[0, 15, 15]], np.int32)
