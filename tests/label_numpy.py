"""The contract of neilpy_amd/label.py restated in NumPy and plain Python (a plain helper module, no test in it, and no
import of the package): union-find to the minimum linear index, numbering of the roots by rank,
sizes, boxes, and the masks the tests are run on, constructed ones and seeded random ones with structure.
tests/test_label_host.py pins it to scipy.ndimage."""
import numpy as np

E, S, SE, SW = 1, 2, 4, 8
FOUR, EIGHT = E | S, E | S | SE | SW


def structure_of(links):
    """the 3 x 3 structure of a 4-bit link mask (centre set, as SciPy's generated structures have it)"""
    s = np.zeros((3, 3), dtype=bool)
    s[1, 1] = True
    for bit, (dr, dc) in ((E, (0, 1)), (S, (1, 0)), (SE, (1, 1)), (SW, (1, -1))):
        if links & bit:
            s[1 + dr, 1 + dc] = s[1 - dr, 1 - dc] = True
    return s


STRUCTURES = [structure_of(k) for k in range(16)]


def links_of(structure):
    """the link mask of a 3 x 3 structure; ValueError where it is not centrally symmetric (the centre is ignored)"""
    s = np.asarray(structure, dtype=bool)
    assert s.shape == (3, 3)
    if not np.array_equal(s, s[::-1, ::-1]):
        raise ValueError("not centrally symmetric")
    return E * bool(s[1, 2]) | S * bool(s[2, 1]) | SE * bool(s[2, 2]) | SW * bool(s[2, 0])


def roots(mask, links):
    """per cell the smallest linear index of its object (-1 for background): union-find in which the larger root always
    hangs below the smaller one"""
    fg = np.asarray(mask) != 0
    rows, cols = fg.shape
    parent = np.where(fg.ravel(), np.arange(fg.size), -1).tolist()

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    offsets = [(dr, dc) for bit, (dr, dc) in ((E, (0, 1)), (S, (1, 0)), (SE, (1, 1)), (SW, (1, -1))) if links & bit]
    for r, c in zip(*np.nonzero(fg)):
        for dr, dc in offsets:
            r2, c2 = r + dr, c + dc
            if r2 < rows and 0 <= c2 < cols and fg[r2, c2]:
                a, b = find(r * cols + c), find(r2 * cols + c2)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(i) if p >= 0 else -1 for i, p in enumerate(parent)], dtype=np.int64).reshape(fg.shape)


def number(root):
    """object k is the one whose root - its first cell in C order - comes k-th: rank of the root among the roots, plus 1"""
    flat = root.ravel()
    firsts = np.flatnonzero(flat == np.arange(flat.size))
    out = np.zeros(flat.size, dtype=np.int32)
    fg = flat >= 0
    out[fg] = np.searchsorted(firsts, flat[fg]) + 1
    return out.reshape(root.shape), int(firsts.size)


def label(mask, structure=None):
    links = FOUR if structure is None else links_of(structure)
    return number(roots(mask, links))


def region_sizes(L, n):
    L = np.asarray(L).ravel()
    return np.array([np.count_nonzero(L == k) for k in range(n + 1)], dtype=np.int64)


def bounding_boxes(L, n):
    L = np.asarray(L)
    out = np.zeros((n, 4), dtype=np.int32)
    for k in range(1, n + 1):
        r, c = np.nonzero(L == k)
        if r.size:
            out[k - 1] = (r.min(), r.max() + 1, c.min(), c.max() + 1)
    return out


def find_objects(L, max_label=0):
    L = np.asarray(L)
    n = max_label if max_label >= 1 else max(int(L.max()), 0)
    return [(slice(int(r0), int(r1), None), slice(int(c0), int(c1), None)) if r1 else None
            for r0, r1, c0, c1 in bounding_boxes(L, n)]


def kept(L, sizes, min_size):
    """``np.isin(L, np.flatnonzero(sizes >= min_size)[1:])``, the expression remove_small_objects' contract is stated in.
    Its ``[1:]`` drops the background, which it takes to pass ``min_size``; where the background is smaller than that
    (one object that fills more than half the raster, at ``min_size`` = its size) nothing is there to drop."""
    big = np.flatnonzero(sizes >= min_size)
    if sizes[0] >= min_size:
        return np.isin(L, big[1:])
    return np.isin(L, big)


def remove_small_objects(mask, min_size, connectivity=1):
    L, n = label(mask, STRUCTURES[FOUR if connectivity == 1 else EIGHT])
    return kept(L, region_sizes(L, n), min_size)


# ------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------
def random_mask(shape, p, seed):
    return np.random.default_rng([20270101, seed, int(p * 100)] + list(shape)).random(shape) < p


def serpentine(shape):
    """every other row full, the rows between them one cell at alternating ends: one object (4-connected) that crosses
    every tile seam many times and whose union chains are the longest"""
    a = np.zeros(shape, dtype=bool)
    a[::2] = True
    a[1::4, -1] = True
    a[3::4, 0] = True
    return a


def spiral(shape):
    """rectangular rings at every other inset, each opened below its top-left corner and joined to the next one inside"""
    rows, cols = shape
    a = np.zeros(shape, dtype=bool)
    k = 0
    while rows - 2 * k >= 1 and cols - 2 * k >= 1:
        r0, r1, c0, c1 = k, rows - 1 - k, k, cols - 1 - k
        a[r0, c0:c1 + 1] = a[r1, c0:c1 + 1] = True
        a[r0:r1 + 1, c1] = a[r0:r1 + 1, c0] = True
        if r0 + 1 <= r1:
            a[r0 + 1, c0] = False                             # the ring is opened ...
        if r0 + 2 <= r1 and c0 + 2 <= c1:
            a[r0 + 2, c0 + 1] = True                          # ... and its end runs into the next ring's corner
        k += 2
    return a


def comb(shape):
    a = np.zeros(shape, dtype=bool)
    a[0] = True
    a[:, ::2] = True
    return a


def stripes(shape, direction):
    """diagonal stripes two cells apart, running south-east (+1) or south-west (-1): diagonal links only"""
    r, c = np.indices(shape)
    return (r - direction * c) % 3 == 0


def u_and_speck(shape):
    """a 'U' whose arms join only in the last row - the right arm starts in row 0, the left one in row 2 - and a speck in
    row 1 between them: the U's first cell is the right arm's, so the U is object 1 and the speck object 2; a labeller
    that numbers by the left arm's first cell swaps them"""
    rows, cols = shape
    a = np.zeros(shape, dtype=bool)
    a[2:, 2] = True
    a[0:, cols - 3] = True
    a[-1, 2:cols - 2] = True
    a[1, cols // 2] = True
    return a


def frame(shape):
    a = np.zeros(shape, dtype=bool)
    a[0] = a[-1] = True
    a[:, 0] = a[:, -1] = True
    return a


def checkerboard(shape):
    r, c = np.indices(shape)
    return (r + c) % 2 == 0


def constructed(shape):
    """name -> mask of the constructed cases"""
    return {"ones": np.ones(shape, dtype=bool), "zeros": np.zeros(shape, dtype=bool), "checkerboard": checkerboard(shape),
            "serpentine": serpentine(shape), "spiral": spiral(shape), "comb": comb(shape), "stripes se": stripes(shape, 1),
            "stripes sw": stripes(shape, -1), "u and speck": u_and_speck(shape), "frame": frame(shape)}


# ------------------------------------------------------------------------------------------
# structured random masks: a shape and a seed each, NumPy and SciPy only, 1 x N and N x 1 included
# ------------------------------------------------------------------------------------------
def _rng(name, shape, seed):
    return np.random.default_rng([20270206, sum(map(ord, name)), seed] + list(shape))


def blobs(shape, seed):
    """box-smoothed noise above its median: solid objects some tens of cells across, with holes, that cross the seams"""
    import scipy.ndimage as ndi
    smooth = ndi.uniform_filter(_rng("blobs", shape, seed).random(shape), size=9, mode="reflect")
    return smooth > np.median(smooth)


def strokes(shape, seed):
    """thick segments at random angles: 1 to 4 cells thick, up to the raster's length long"""
    rng = _rng("strokes", shape, seed)
    rows, cols = shape
    a = np.zeros(shape, dtype=bool)
    t = np.linspace(0.0, 1.0, 2 * max(rows, cols) + 1)
    for _ in range(4 + (rows + cols) // 16):
        (r0, r1), (c0, c1), thick = rng.random(2) * (rows - 1), rng.random(2) * (cols - 1), int(rng.integers(1, 5))
        r, c = np.rint(r0 + (r1 - r0) * t).astype(int), np.rint(c0 + (c1 - c0) * t).astype(int)
        for dr in range(thick):
            for dc in range(thick):
                a[np.minimum(r + dr, rows - 1), np.minimum(c + dc, cols - 1)] = True
    return a


def rings(shape, seed):
    """concentric rings about a drawn centre, 1 to 4 cells wide and as far apart: objects in the holes of others"""
    rng = _rng("rings", shape, seed)
    r, c = np.indices(shape)
    width = int(rng.integers(1, 5))
    d = np.hypot(r - rng.random() * (shape[0] - 1), c - rng.random() * (shape[1] - 1))
    return np.floor(d / width).astype(np.int64) % 2 == 0


def maze(shape, seed):
    """a random spanning tree of the cells at even rows and columns, the passages between joined cells opened: one
    4-connected object of one-cell corridors with no loop, so its union chains are long and winding"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    rng = _rng("maze", shape, seed)
    rows, cols = shape
    gr, gc = (rows + 1) // 2, (cols + 1) // 2
    node = np.arange(gr * gc).reshape(gr, gc)
    a = np.zeros(shape, dtype=bool)
    a[::2, ::2] = True
    u = np.concatenate([node[:, :-1].ravel(), node[:-1, :].ravel()])
    v = np.concatenate([node[:, 1:].ravel(), node[1:, :].ravel()])
    if u.size:
        tree = minimum_spanning_tree(coo_matrix((rng.random(u.size) + 0.5, (u, v)), shape=(node.size, node.size))).tocoo()
        a[tree.row // gc + tree.col // gc, tree.row % gc + tree.col % gc] = True       # the cell between the two
    return a


GENERATORS = {f.__name__: f for f in (blobs, strokes, rings, maze)}


# a hand-made label raster: gaps (3 and 6 do not occur), a label above any max_label a test passes (40), negative cells
HAND = np.array([[0, 1, 1, 0, 0, -3, 7],
                 [0, 0, 1, 0, 2, 2, 7],
                 [5, 0, 0, 0, 0, 2, 0],
                 [5, 5, 0, 40, 0, 0, 4],
                 [0, 5, -1, 40, 4, 4, 4]], dtype=np.int32)
