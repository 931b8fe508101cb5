"""A drawn table of flat footprints for grey morphology and the rank filters - TEST INFRASTRUCTURE, pure NumPy, no test in
it (DESIGN.md sections 19 and 20).  tests/test_footprint_draws_host.py runs the table through a NumPy model of the runs
kernel and asserts what the table covers; tests/test_gpu_draws.py launches it.

A case is ``(id, raster shape, dtype, mode, spec, nan)`` and a spec a literal ``(kind, params...)`` that ``build`` turns
into a footprint:

``("runs", kh, kw, ((row, ((col0, length), ...)), ...))``   maximal runs of members, gaps between them;
``("bernoulli", kh, kw, density, seed)``                    ``default_rng(seed).random((kh, kw)) < density``;
``("thin", kh, kw, density, seed)``                         the same on a box 1 to 3 cells wide or high, 1.0 = all ones;
``("margin", kh, kw, row0, col0, inner)``                   the footprint of the spec ``inner`` at (row0, col0) of an
                                                            otherwise empty kh x kw array;
``("far", kh, kw, ((row, col), ...))``                      single members, up to morphology.MAX_EXTENT apart.

A Bernoulli draw without a member gets the centre of its box.

The cases were drawn once from numpy's default_rng(20270201) and are kept as literals, so a failure names its case and
replays alone: run lengths from RUN_LENGTHS with 1 to 6 sample rows; Bernoulli boxes of 1..40 x 1..90 at DENSITIES; thin
boxes of THIN_LONG x 1..3 and their transposes, all ones and at 70 %; margins on one to four sides, a single off-centre
member (a pure shift) and two members in opposite corners among them; far members at FAR_EXTENTS on FAR_RASTERS in both
modes.  Rasters have rows from ROWS and columns from COLS, cells x members <= MAX_WORK (the bound under which
rank_numpy.samples stays cheap, so both families run every case), and a fifth of the cases hold 5 % NaN."""
import numpy as np

RUN_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129)
DENSITIES = (0.05, 0.3, 0.6, 0.95)
THIN_LONG = (9, 17, 33, 65, 130, 200)
FAR_EXTENTS = ((1, 1 << 20), (1 << 20, 1), (4097, 4097))
FAR_RASTERS = ((9, 65), (70, 129))
ROWS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 70, 150)
COLS = (1, 2, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 300)
KINDS = ("runs", "bernoulli", "thin", "margin", "far")
DTYPES = {"f32": np.float32, "f64": np.float64}
MAX_WORK = 4e6
NAN = 0.05


def build(spec):
    """the footprint of a spec, as a uint8 array"""
    kind, kh, kw = spec[:3]
    fp = np.zeros((kh, kw), dtype=np.uint8)
    if kind == "runs":
        for row, runs in spec[3]:
            for col0, length in runs:
                assert not fp[row, max(col0 - 1, 0):col0 + length + 1].any(), spec        # maximal, a gap on both sides
                fp[row, col0:col0 + length] = 1
    elif kind in ("bernoulli", "thin"):
        density, seed = spec[3:]
        fp[:] = 1 if density == 1.0 else np.random.default_rng(seed).random((kh, kw)) < density
        if not fp.any():
            fp[kh // 2, kw // 2] = 1
    elif kind == "margin":
        row0, col0, inner = spec[3:]
        part = build(inner)
        fp[row0:row0 + part.shape[0], col0:col0 + part.shape[1]] = part
    elif kind == "far":
        for row, col in spec[3]:
            fp[row, col] = 1
    else:
        raise ValueError("unknown kind %r" % (kind,))
    assert fp.any(), spec
    return fp


def box(fp):
    """rows and columns of the members' bounding box"""
    s, t = np.nonzero(fp)
    return int(s.max() - s.min() + 1), int(t.max() - t.min() + 1)


def inputs(case):
    """the raster (tests/test_gpu_footprint.py's, seeded by the case's id) and the footprint of a case"""
    from test_gpu_footprint import raster
    cid, shape, dtype, mode, spec, nan = case
    return raster(np.random.default_rng([20270202, cid]), shape, DTYPES[dtype], NAN if nan else 0.0), build(spec)


CASES = [
    # id, raster shape, dtype, mode, spec, nan
    (500, (150, 64), 'f32', 'reflect', ('runs', 2, 3, ((0, ((0, 1), (2, 1))),)), False),
    (501, (65, 193), 'f64', 'reflect', ('runs', 4, 17, ((0, ((2, 3), (8, 3))), (1, ((4, 1), (7, 2), (10, 1))), (3, ((3, 3), (10, 3), (16, 1))))), False),
    (502, (64, 2), 'f32', 'nearest', ('runs', 2, 9, ((0, ((3, 5),)),)), False),
    (503, (70, 127), 'f64', 'nearest', ('runs', 4, 28, ((0, ((2, 9), (13, 5), (21, 7))), (2, ((0, 9), (13, 9))), (3, ((2, 2), (7, 4))))), True),
    (504, (2, 2), 'f32', 'reflect', ('runs', 9, 20, ((0, ((3, 17),)), (1, ((1, 7),)), (3, ((0, 16),)), (5, ((2, 8),)), (7, ((3, 2),)), (8, ((3, 3), (7, 7))))), False),
    (505, (9, 300), 'f64', 'reflect', ('runs', 9, 113, ((0, ((3, 33), (41, 33), (79, 33))), (3, ((1, 8), (13, 4), (18, 17))), (4, ((0, 33),)), (6, ((2, 31),)), (7, ((4, 5), (11, 32))))), False),
    (506, (16, 191), 'f32', 'nearest', ('runs', 7, 172, ((0, ((0, 100),)), (1, ((1, 65), (71, 100))), (4, ((1, 63),)), (5, ((1, 2), (6, 4))), (6, ((0, 32), (33, 100))))), False),
    (507, (2, 65), 'f64', 'nearest', ('runs', 1, 130, ((0, ((1, 129),)),)), False),
    (508, (16, 130), 'f32', 'reflect', ('runs', 2, 14, ((0, ((0, 1), (6, 1), (12, 1))),)), True),
    (509, (64, 193), 'f64', 'reflect', ('runs', 7, 11, ((0, ((0, 3),)), (1, ((1, 2), (4, 3), (9, 1))), (2, ((3, 2),)), (5, ((4, 1), (7, 3))))), False),
    (510, (2, 127), 'f32', 'nearest', ('runs', 3, 8, ((0, ((3, 5),)), (2, ((0, 5), (6, 2))))), False),
    (511, (64, 127), 'f64', 'nearest', ('runs', 9, 23, ((0, ((0, 9), (14, 9))), (3, ((3, 7),)), (6, ((0, 8),)), (7, ((1, 2), (7, 7))))), False),
    (512, (2, 1), 'f32', 'reflect', ('runs', 8, 48, ((0, ((4, 17), (26, 1), (32, 16))), (3, ((0, 2),)), (6, ((0, 9), (12, 4))), (7, ((2, 16), (23, 17), (45, 2))))), False),
    (513, (70, 64), 'f64', 'reflect', ('runs', 5, 49, ((0, ((0, 33),)), (3, ((1, 4), (10, 9))), (4, ((1, 8), (11, 3), (16, 32))))), True),
    (514, (15, 192), 'f32', 'nearest', ('runs', 2, 114, ((0, ((2, 100), (107, 2), (111, 3))),)), False),
    (515, (16, 128), 'f64', 'nearest', ('runs', 5, 139, ((0, ((0, 129), (134, 5))), (2, ((3, 128),)), (4, ((0, 33), (36, 33))))), False),
    (516, (64, 127), 'f32', 'reflect', ('bernoulli', 11, 13, 0.05, 1029805537), False),
    (517, (1, 130), 'f64', 'reflect', ('bernoulli', 10, 74, 0.3, 493908709), False),
    (518, (63, 193), 'f32', 'nearest', ('bernoulli', 30, 10, 0.6, 284956393), True),
    (519, (16, 1), 'f64', 'nearest', ('bernoulli', 26, 36, 0.95, 795489747), False),
    (520, (70, 192), 'f32', 'reflect', ('bernoulli', 12, 63, 0.05, 266982354), False),
    (521, (9, 300), 'f64', 'reflect', ('bernoulli', 36, 90, 0.3, 34933115), False),
    (522, (7, 127), 'f32', 'nearest', ('bernoulli', 15, 58, 0.6, 796863106), False),
    (523, (8, 191), 'f64', 'nearest', ('bernoulli', 34, 61, 0.95, 163662945), True),
    (524, (1, 300), 'f32', 'reflect', ('bernoulli', 10, 7, 0.05, 60370198), False),
    (525, (15, 191), 'f64', 'reflect', ('bernoulli', 30, 2, 0.3, 679658766), False),
    (526, (1, 65), 'f32', 'nearest', ('bernoulli', 7, 88, 0.6, 649430098), False),
    (527, (7, 300), 'f64', 'nearest', ('bernoulli', 27, 14, 0.95, 614868152), False),
    (528, (8, 300), 'f32', 'reflect', ('bernoulli', 8, 51, 0.05, 885210669), True),
    (529, (63, 1), 'f64', 'reflect', ('bernoulli', 11, 32, 0.3, 781094907), False),
    (530, (65, 63), 'f32', 'nearest', ('thin', 9, 1, 1.0, 332267283), False),
    (531, (64, 191), 'f64', 'nearest', ('thin', 2, 9, 0.7, 261490786), False),
    (532, (15, 130), 'f32', 'reflect', ('thin', 17, 2, 0.7, 335421654), False),
    (533, (64, 1), 'f64', 'reflect', ('thin', 3, 17, 1.0, 915346321), True),
    (534, (15, 193), 'f32', 'nearest', ('thin', 33, 3, 1.0, 404477322), False),
    (535, (150, 300), 'f64', 'nearest', ('thin', 1, 33, 0.7, 808305081), False),
    (536, (17, 193), 'f32', 'reflect', ('thin', 65, 1, 0.7, 965436323), False),
    (537, (8, 64), 'f64', 'reflect', ('thin', 2, 65, 1.0, 158722404), False),
    (538, (150, 64), 'f32', 'nearest', ('thin', 130, 2, 1.0, 87643247), True),
    (539, (63, 191), 'f64', 'nearest', ('thin', 3, 130, 0.7, 130796616), False),
    (540, (15, 191), 'f32', 'reflect', ('thin', 200, 3, 0.7, 1064472599), False),
    (541, (8, 127), 'f64', 'reflect', ('thin', 1, 200, 1.0, 596243646), False),
    (542, (150, 65), 'f32', 'nearest', ('margin', 6, 2, 5, 1, ('far', 1, 1, ((0, 0),))), False),
    (543, (17, 300), 'f64', 'nearest', ('margin', 4, 4, 0, 0, ('far', 1, 1, ((0, 0),))), True),
    (544, (63, 128), 'f32', 'reflect', ('margin', 20, 42, 5, 1, ('far', 9, 33, ((0, 0), (8, 32)))), False),
    (545, (16, 192), 'f64', 'reflect', ('margin', 20, 9, 0, 0, ('far', 20, 5, ((0, 4), (19, 0)))), False),
    (546, (70, 65), 'f32', 'nearest', ('margin', 10, 9, 5, 0, ('bernoulli', 5, 9, 0.6, 196630279)), False),
    (547, (150, 128), 'f64', 'nearest', ('margin', 7, 48, 0, 8, ('bernoulli', 3, 40, 0.3, 554438126)), False),
    (548, (70, 63), 'f32', 'reflect', ('margin', 19, 13, 3, 1, ('bernoulli', 12, 12, 0.95, 245828204)), True),
    (549, (15, 193), 'f64', 'reflect', ('margin', 15, 84, 8, 7, ('runs', 2, 70, ((0, ((0, 65),)), (1, ((3, 4), (9, 61)))))), False),
    (550, (9, 65), 'f32', 'reflect', ('far', 1, 1048576, ((0, 0), (0, 524285), (0, 1048575))), False),
    (551, (9, 65), 'f64', 'nearest', ('far', 1, 1048576, ((0, 0), (0, 17960), (0, 747382), (0, 1048575))), False),
    (552, (70, 129), 'f64', 'reflect', ('far', 1, 1048576, ((0, 0), (0, 524286), (0, 524287), (0, 524291), (0, 1048575))), False),
    (553, (70, 129), 'f32', 'nearest', ('far', 1, 1048576, ((0, 0), (0, 459162), (0, 1048575))), True),
    (554, (9, 65), 'f64', 'reflect', ('far', 1048576, 1, ((0, 0), (524287, 0), (1048575, 0))), False),
    (555, (9, 65), 'f32', 'nearest', ('far', 1048576, 1, ((0, 0), (176381, 0), (1048575, 0))), False),
    (556, (70, 129), 'f32', 'reflect', ('far', 1048576, 1, ((0, 0), (524287, 0), (524288, 0), (524291, 0), (1048575, 0))), False),
    (557, (70, 129), 'f64', 'nearest', ('far', 1048576, 1, ((0, 0), (1048575, 0))), False),
    (558, (9, 65), 'f32', 'reflect', ('far', 4097, 4097, ((0, 0), (0, 4096), (3485, 1995), (3711, 116))), True),
    (559, (9, 65), 'f64', 'nearest', ('far', 4097, 4097, ((2046, 2046), (2919, 3809), (3781, 2723), (4096, 0), (4096, 4096))), False),
    (560, (70, 129), 'f64', 'reflect', ('far', 4097, 4097, ((0, 4096), (4096, 0), (4096, 4096))), False),
    (561, (70, 129), 'f32', 'nearest', ('far', 4097, 4097, ((0, 0), (0, 4096), (2047, 2046), (2049, 2050), (4096, 0))), False),
]

IDS = [str(case[0]) for case in CASES]
