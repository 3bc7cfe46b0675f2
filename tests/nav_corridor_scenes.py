"""Hand-built volumes for the free boxes and corridors (tests/test_nav_corridor_cpu.py, tests/test_nav_corridor_gpu.py): the smallest shapes at which
tsl_nav_corridor.hip can still go wrong.  WALL marks a cell that is not free under the default free_below of 253.  A box scene is (name, cost u8
[D, H, W], cells int32 [S, 3], free_below, ext); a corridor scene is (name, cost, cells int16 [P, L, 3], length int32 [P], free_below, ext, max_boxes).
The kernel packs a row into 64-bit words, so the widths sit around 64, and it loops a wave over the items of a slab -- (k, i) pairs for the +-j faces,
(row, word) pairs for the +-i and +-k faces -- so some slabs of either kind have more than 64 items (tests/test_nav_corridor_cpu.py counts them with
nav_corridor_ref.tries)."""
import numpy as np

WALL = 254
FREE_BELOW = 253
WIDTHS = (1, 63, 64, 65, 70)


def random_volume(D, H, W, share=0.03, seed=7):
    rng = np.random.default_rng(seed + 1000 * D + 10 * H + W)
    cost = rng.integers(0, 200, (D, H, W)).astype(np.uint8)
    cost[rng.random((D, H, W)) < share] = WALL
    return cost


def probe_cells(shape, n_random=24, seed=3):
    """seeds on every corner and face centre of the volume, outside on every side, negative and far away, and some anywhere"""
    D, H, W = shape
    rng = np.random.default_rng(seed + D + H + W)
    c = [[k, i, j] for k in (0, D - 1) for i in (0, H - 1) for j in (0, W - 1)]
    c += [[0, H // 2, W // 2], [D - 1, H // 2, W // 2], [D // 2, 0, W // 2], [D // 2, H - 1, W // 2], [D // 2, H // 2, 0], [D // 2, H // 2, W - 1]]
    c += [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [D, 0, 0], [0, H, 0], [0, 0, W], [-5, -5, -5], [2 ** 31 - 1, 0, 0], [0, 0, -2 ** 31], [D // 2, H // 2, W + 63]]
    c += np.stack([rng.integers(0, D, n_random), rng.integers(0, H, n_random), rng.integers(0, W, n_random)], 1).tolist()
    return np.array(c, np.int32)


def width_scene(W):
    """a plane of two layers whose rows end in a partial word (or a full one), with walls at the word border: boxes straddle bit 63 / 64"""
    D, H = 2, 9
    cost = random_volume(D, H, W, share=0.04, seed=11)
    cells = probe_cells((D, H, W), 12)
    near = [[d, i, j] for d in (0, 1) for i in (0, 4, 8) for j in (W - 1, W - 2, 62, 63, 64, 65) if 0 <= j < W]
    cells = np.concatenate([cells, np.array(near, np.int32).reshape(-1, 3)])
    return (f"width {W}", cost, cells, FREE_BELOW, (1, 4, 40))


def wide_plane():
    """1 x 80 x 150 with ext 127: a j-run over three words for the +-i slabs, and +-j slabs of up to 80 cells, more than a wave"""
    cost = np.zeros((1, 80, 150), np.uint8)
    cost[0, 10, 140] = cost[0, 70, 3] = cost[0, 40, 75] = WALL
    cells = np.array([[0, 40, 70], [0, 40, 76], [0, 0, 0], [0, 79, 149], [0, 11, 139], [0, 69, 4], [0, 40, 75], [0, 20, 64], [0, 60, 63], [0, 39, 128]], np.int32)
    return ("wide plane 1 x 80 x 150, ext 127", cost, cells, FREE_BELOW, (0, 127, 127))


def tall_plane():
    """150 rows: a +-j slab of more than 64 rows in a plane, and a +-i slab of one row over three words"""
    cost = np.zeros((1, 150, 80), np.uint8)
    cost[0, 140, 10] = cost[0, 3, 70] = WALL
    cells = np.array([[0, 75, 40], [0, 0, 0], [0, 149, 79], [0, 139, 11], [0, 4, 69]], np.int32)
    return ("tall plane 1 x 150 x 80, ext 127", cost, cells, FREE_BELOW, (0, 127, 127))


def cube12():
    """12 x 12 x 12 with ext 5: the largest +-j slab tried has 81 (k, i) pairs, more than a wave (j closes on ext while k and i span 9; the finished box
    is 11 x 11 across); the +-k / +-i slabs have up to 11 rows of one word"""
    cost = np.zeros((12, 12, 12), np.uint8)
    cost[0, 0, 0] = cost[11, 11, 11] = cost[6, 0, 11] = WALL
    cells = np.array([[6, 6, 6], [5, 5, 5], [6, 5, 6], [1, 1, 1], [10, 10, 10], [6, 1, 10], [0, 0, 0], [0, 6, 6], [6, 6, 0]], np.int32)
    return ("cube 12 x 12 x 12, ext 5", cost, cells, FREE_BELOW, (5, 5, 5))


def deep_slabs():
    """70 x 70 x 70 with ext 34 and seeds beside the word border at column 64.  The faces of a round are tried as j, i, k, so in round r a +-i slab has
    2 r - 1 layers and a +-k slab 2 r + 1 rows, each a run over two words: from round 17 on more than 64 (row, word) items, 134 and 138 at the end.  (A
    slab of the +-i or +-k faces gets many rows only while BOTH other axes keep growing: a thin volume closes the short axis in the first rounds, and
    the issue's 1 x 80 x 150 plane has one-row slabs for +-i.)  One wall fails a +-k try in its second pass."""
    cost = np.zeros((70, 70, 70), np.uint8)
    cost[69, 60, 40] = cost[0, 0, 0] = WALL                        # (69, 60, 40): row 60 - 1 = 59 of the +k slab at layer 69, item 59 * 2 + 0 = 118
    cells = np.array([[35, 35, 63], [35, 35, 64], [34, 34, 66], [35, 35, 10], [1, 1, 1]], np.int32)
    return ("deep slabs 70 x 70 x 70, ext 34", cost, cells, FREE_BELOW, (34, 34, 34))


def broad_slabs():
    """200 x 20 x 260 with ext 127 and a seed at column 159: i closes on the border after ten rounds, j and k keep growing, and from round 97 on the
    run j0 .. j1 spans five words (62 .. 256): a +-k slab is then 20 rows x 5 words = 100 items, two passes of the wave with the item -> (row, word)
    split at every remainder.  The wall at (0, 15, 200) makes the -k try at layer 0 fail at item 15 * 5 + 3 = 78, in the second pass.  Other seeds give
    runs of three and four words."""
    cost = np.zeros((200, 20, 260), np.uint8)
    cost[0, 15, 200] = cost[199, 3, 5] = WALL
    cells = np.array([[100, 10, 159], [100, 10, 130], [99, 5, 100], [60, 10, 200]], np.int32)
    return ("broad slabs 200 x 20 x 260, ext 127", cost, cells, FREE_BELOW, (127, 127, 127))


def empty_volume():
    """nothing blocks: the box is the volume clipped to ext, here the whole volume"""
    cost = np.zeros((5, 7, 9), np.uint8)
    return ("empty 5 x 7 x 9, ext 20", cost, probe_cells(cost.shape, 8), FREE_BELOW, (20, 20, 20))


def zero_ext(axis):
    cost = random_volume(6, 11, 13, share=0.02, seed=5)
    ext = [4, 4, 4]
    ext[axis] = 0
    return (f"ext 0 on axis {axis}", cost, probe_cells(cost.shape, 16), FREE_BELOW, tuple(ext))


def l_shape():
    """A 1 x 5 x 5 plane whose free cells are column 0 and row 4: an L with its corner at (4, 0).  From the corner the faces are tried as -j (outside),
    +j (row 4, column 1: free -> moves), -i (row 3, columns 0 .. 1: (3, 1) is a wall -> closes for good) ..: the box runs along row 4.  Had -i come
    first the box would run up column 0.  With ext_j = 0 the +-j faces close at once and the box does run up column 0."""
    cost = np.full((1, 5, 5), WALL, np.uint8)
    cost[0, :, 0] = 0
    cost[0, 4, :] = 0
    return cost


L_SHAPE_CASES = (((0, 4, 0), (0, 4, 4), [0, 4, 0, 0, 4, 4], 0),      # the corner: along the row, because -j / +j come first
                 ((0, 4, 0), (0, 4, 0), [0, 0, 0, 0, 4, 0], 0),      # the corner without reach in j: up the column
                 ((0, 2, 0), (0, 4, 4), [0, 0, 0, 0, 4, 0], 0),      # in the column: +j fails on (2, 1) in round 1, so row 4 is only ever tested at column 0
                 ((0, 4, 3), (0, 4, 2), [0, 4, 1, 0, 4, 4], 0),      # in the row, reach 2: columns 1 .. 4 (5 is outside)
                 ((0, 1, 1), (0, 4, 4), [0, 1, 1, 0, 1, 1], 1),      # a wall
                 ((0, 5, 0), (0, 4, 4), [-1] * 6, 2))                # outside


def free_below_cases():
    """free_below 1: only cost 0 is free; free_below 255: everything but 255"""
    cost = random_volume(3, 9, 20, share=0.0, seed=9)
    cost[cost < 40] = 0
    cost[1, 4, 10] = 255
    cost[1, 4, 11] = 254
    cells = probe_cells(cost.shape, 20)
    return [("free_below 1", cost, cells, 1, (1, 3, 6)), ("free_below 255", cost, cells, 255, (1, 3, 6))]


RANDOM_SHAPE = (20, 37, 70)
RANDOM_EXT = (3, 5, 9)


def random_scene():
    cost = random_volume(*RANDOM_SHAPE)
    return ("random 20 x 37 x 70", cost, probe_cells(cost.shape, 40), FREE_BELOW, RANDOM_EXT)


def box_scenes():
    out = [width_scene(W) for W in WIDTHS]
    out += [wide_plane(), tall_plane(), cube12(), deep_slabs(), broad_slabs(), empty_volume(), zero_ext(0), zero_ext(1), zero_ext(2)]
    cells = np.array([c for c, _, _, _ in L_SHAPE_CASES], np.int32)
    out += [("L shape, ext (0, 4, 4)", l_shape(), cells, FREE_BELOW, (0, 4, 4)), ("L shape, ext (0, 4, 0)", l_shape(), cells, FREE_BELOW, (0, 4, 0))]
    out += free_below_cases()
    out.append(random_scene())
    return out


# ---- corridors ----------------------------------------------------------------------------------------------------------------------------------
def _paths(rows, L):
    """rows: lists of cells -> cells int16 [P, L, 3] (-1 past the end), length int32 [P]"""
    cells = np.full((len(rows), L, 3), -1, np.int16)
    length = np.zeros(len(rows), np.int32)
    for p, r in enumerate(rows):
        if len(r):
            cells[p, :len(r)] = np.array(r, np.int16)
        length[p] = len(r)
    return cells, length


def touch_only():
    """A 1 x 6 x 6 plane, ext (0, 1, 1), walls at (row 3, col 1) and (row 2, col 4), the path (2, 2) -> (3, 3).  The box of (2, 2): -j and +j move
    (columns 1 .. 3), -i moves (row 1, columns 1 .. 3 are free), +i fails on (3, 1): rows 1 .. 2.  The box of (3, 3): columns 2 .. 4, -i fails on
    (2, 4), +i moves: rows 3 .. 4.  The two boxes only touch: link 2."""
    cost = np.zeros((1, 6, 6), np.uint8)
    cost[0, 3, 1] = cost[0, 2, 4] = WALL
    cells, length = _paths([[[0, 2, 2], [0, 3, 3]]], 4)
    return ("touch only", cost, cells, length, FREE_BELOW, (0, 1, 1), 4)


TOUCH_ONLY_WANT = {"boxes": [[0, 1, 1, 0, 2, 3], [0, 3, 2, 0, 4, 4]], "seed": [0, 1], "link": [0, 2], "count": 2, "status": 0}


def blocked_middle():
    """a straight path over a cell that is free for the field (cost 200 < lethal) but not for the corridor (free_below 100)"""
    cost = np.zeros((1, 5, 12), np.uint8)
    cost[0, 2, 6] = 200
    row = [[0, 2, j] for j in range(12)]
    cells, length = _paths([row], 12)
    return ("blocked middle", cost, cells, length, 100, (0, 2, 3), 12)


def cut_at_max_boxes():
    name, cost, cells, length, fb, ext, _ = blocked_middle()
    return ("cut at max_boxes", cost, cells, length, fb, ext, 2)


def short_paths():
    """lengths 0 and 1, a negative length, a length above L, a path that starts outside, one that repeats a cell, and one that leaves the volume midway"""
    cost = random_volume(4, 9, 30, share=0.05, seed=2)
    rows = [[], [[1, 4, 4]], [[1, 4, 4], [1, 4, 5]], [[1, 4, j] for j in range(8)], [[-1, 0, 0], [0, 0, 0], [0, 1, 1]], [[2, 3, 3], [2, 3, 3], [2, 3, 4]],
            [[0, 0, 27], [0, 0, 28], [0, 0, 29], [0, 0, 30], [0, 1, 29]]]
    cells, length = _paths(rows, 8)
    length[2] = -3
    length[3] = 100
    return ("short paths", cost, cells, length, FREE_BELOW, (1, 2, 4), 5)


def straight_random():
    """the random volume with straight and diagonal runs through it, walls included"""
    cost = random_volume(*RANDOM_SHAPE)
    D, H, W = RANDOM_SHAPE
    rows = [[[10, 18, j] for j in range(W)], [[k, 5, 40] for k in range(D)], [[3, i, 66] for i in range(H)], [[t, t, t] for t in range(D)],
            [[7, 36 - t, 2 * t] for t in range(35)], [[19, 0, j] for j in range(W - 1, -1, -1)]]
    cells, length = _paths(rows, W)
    return ("straight runs through the random volume", cost, cells, length, FREE_BELOW, RANDOM_EXT, 40)


def wide_corridor():
    """the 1 x 80 x 150 plane with ext 127 and a path of 150 cells: the chain's ballots run over three groups of 64 cells"""
    _, cost, _, _, _ = wide_plane()
    rows = [[[0, 40, j] for j in range(150)], [[0, min(79, j), j] for j in range(150)]]
    cells, length = _paths(rows, 150)
    return ("wide corridor", cost, cells, length, FREE_BELOW, (0, 127, 127), 16)


def corridor_scenes():
    return [touch_only(), blocked_middle(), cut_at_max_boxes(), short_paths(), straight_random(), wide_corridor()]
