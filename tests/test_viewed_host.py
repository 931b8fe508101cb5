"""The view harness (tests/viewed.py) proves itself on the CPU: stand-ins, plain torch ops on the harness's own buffers,
handle a view rightly or wrongly in each of the ways the harness is there to detect, and every check fails when it
should, for its stated reason, and passes when it should.  The layout constructors are tested on their own."""
import numpy as np
import pytest
import torch

import viewed as V
from viewed import IdentityError, InputsError, ResultsError, SurroundingsError, run_viewed

SHAPES = ((1, 1), (1, 65), (65, 1), (67, 131))
DTYPES = (np.uint8, np.float32, np.float64)


# ------------------------------------------------------------------------------------------
# stand-ins
# ------------------------------------------------------------------------------------------
def _strides(shape):
    out, n = [], 1
    for v in reversed(shape):
        out.append(n)
        n *= v
    return tuple(reversed(out))


def _cells(t):
    """the storage behind ``t`` as one flat tensor: the address space a kernel given ``t.data_ptr()`` works in"""
    return torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)


def double(bug=None):
    """out = 2 * x + 1.  ``base``: reads from the buffer's base instead of the view; ``contiguous``: reads the view as
    if it were contiguous from its first element; ``past`` / ``before``: also writes one element past the view's last /
    before its first, where the storage has such a cell"""
    def fn(x):
        host = isinstance(x, np.ndarray)
        t = torch.from_numpy(np.array(x, order="C")) if host else x
        if bug == "base":
            src = torch.as_strided(t, t.shape, _strides(t.shape), 0)
        elif bug == "contiguous":
            src = torch.as_strided(t, t.shape, _strides(t.shape))
        else:
            src = t.contiguous()
        out = 2 * src + 1
        if bug in ("past", "before"):
            flat = _cells(t)
            first = t.storage_offset()
            last = first + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
            at = last + 1 if bug == "past" else first - 1
            if 0 <= at < flat.numel():
                flat[at] = 7
        return out.numpy() if host else out
    return fn


def fill(bug=None):
    """NaN cells become 0 in place, the argument is returned.  ``copy``: a view that is not contiguous is filled in a
    copy that never comes back; ``none``: the same, and nothing is returned"""
    def fn(x):
        if isinstance(x, np.ndarray):
            work = np.array(x, order="C")
            work[np.isnan(work)] = 0
            if not bug:
                x[...] = work
        else:
            work = x.contiguous()                         # x itself when it is contiguous
            work[torch.isnan(work)] = 0
            if work is not x and not bug:
                x.copy_(work)
        return None if bug == "none" else x
    return fn


def same(bug=None):
    """a copy of the argument.  ``alias``: a new tensor on the argument's memory"""
    def fn(x):
        if isinstance(x, np.ndarray):
            return x[...] if bug else np.array(x, order="C")
        return x[...] if bug else x.clone(memory_format=torch.contiguous_format)
    return fn


def raster(shape=(67, 131), dtype=np.float64, nan=False):
    a = np.random.default_rng(20261301).normal(100.0, 5.0, shape).astype(dtype)
    if nan:
        a[np.random.default_rng(5).random(shape) < 0.1] = np.nan
    return a


def run(fn, a, layouts=V.LAYOUTS, **k):
    return run_viewed(fn, [a], name="stand-in", device="cpu", layouts=layouts, **k)


# ------------------------------------------------------------------------------------------
# the harness on them
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES + ((257,), (257, 2), (8, 8, 3)))
def test_a_correct_standin_passes_every_layout(shape, dtype):
    a = raster(shape, dtype)
    stats, seen = {}, []
    plain, ran = run(double(), a, reference=seen.append, stats=stats)
    assert np.array_equal(plain, 2 * a + 1) and seen[0] is plain
    want = [lay for lay in V.LAYOUTS if lay in ("offset", "readonly") or V.carve(shape, a.itemsize, lay)[2] == lay]
    assert ran == want and stats["runs"] == 2 * len(ran), (ran, stats)
    if shape == (67, 131):
        assert ran == list(V.LAYOUTS)


def test_a_correct_fill_passes_every_layout_but_readonly():
    a = raster(nan=True)
    plain, ran = run(fill(), a, known=lambda i, x: ~np.isnan(x))
    assert ran == [lay for lay in V.LAYOUTS if lay != "readonly"]
    assert not np.isnan(plain).any() and np.array_equal(plain[~np.isnan(a)], a[~np.isnan(a)])
    assert run(same(), a)[1] == list(V.LAYOUTS)                 # NaN cells compare as bits


@pytest.mark.parametrize("layout", ["offset", "strided"])
def test_reading_from_the_buffers_base_fails_identity(layout):
    with pytest.raises(IdentityError, match="bytes differ"):
        run(double("base"), raster(), [layout])


@pytest.mark.parametrize("layout", ["strided", "transposed"])
def test_reading_the_view_as_if_contiguous_fails_identity(layout):
    a = raster()
    run(double("contiguous"), a, ["offset"])                   # a contiguous view is what it takes it for
    with pytest.raises(IdentityError, match="bytes differ"):
        run(double("contiguous"), a, [layout])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["offset", "strided"])
@pytest.mark.parametrize("bug", ["past", "before"])
def test_a_write_one_element_past_either_end_fails_surroundings(bug, layout, dtype):
    a = raster(dtype=dtype)
    with pytest.raises(SurroundingsError, match="%d bytes of input 0" % a.itemsize):
        run(double(bug), a, [layout])
    v = V.View(raster((257,), dtype), "strided", 0x5A, "cpu")   # a vector's strided view has a cell on either side too
    assert v.idx[0] == 1 and v.idx[-1] == v.total - 2


@pytest.mark.parametrize("bug", ["copy", "none"])
def test_a_fill_that_stays_in_a_copy_fails_inputs(bug):
    a = raster(nan=True)
    known = lambda i, x: ~np.isnan(x)                           # noqa: E731
    run(fill(bug), a, ["offset"], known=known)                  # contiguous: filled where it lies
    for layout in ("strided", "transposed", "fortran", "reversed"):
        with pytest.raises(InputsError, match="the fill did not arrive in the view"):
            run(fill(bug), a, [layout], known=known)


def test_a_fill_of_known_cells_fails_inputs():
    a = raster(nan=True)
    with pytest.raises(InputsError, match="the plain call changed known cells"):
        run(fill(), a, known=lambda i, x: np.ones(x.shape, bool))

    def scribbles(x):                                           # is to leave its input alone, and does not in a strided view
        out = same()(x)
        if not isinstance(x, np.ndarray) and not x.is_contiguous():
            x[0, 0] = -1.0
        return out
    run(scribbles, a, ["offset"])
    with pytest.raises(InputsError, match="input 0 does not hold"):
        run(scribbles, a, ["strided"])


@pytest.mark.parametrize("layout", V.LAYOUTS)
def test_a_result_in_the_inputs_buffer_fails_results(layout):
    with pytest.raises(ResultsError, match="shares the buffer of input 0|is not contiguous"):
        run(same("alias"), raster(), [layout])
    if layout == "offset":
        with pytest.raises(ResultsError, match="shares the buffer of input 0"):
            run(same("alias"), raster(), [layout])


def test_other_results_that_fail():
    a = raster()
    with pytest.raises(ResultsError, match="is not contiguous"):
        run(lambda x: (2 * x.contiguous()).t().contiguous().t() if not isinstance(x, np.ndarray) else 2 * x, a, ["offset"])
    with pytest.raises(ResultsError, match="is a tensor, NumPy went in"):
        run(lambda x: 2 * (torch.from_numpy(np.array(x, order="C")) if isinstance(x, np.ndarray) else x.contiguous()), a,
            ["fortran"])
    with pytest.raises(IdentityError, match="float32"):
        run(lambda x: double()(x) if not isinstance(x, np.ndarray) else double()(x).astype(np.float32), a, ["reversed"])


# ------------------------------------------------------------------------------------------
# the layouts
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + (np.int64, np.bool_))
def test_offset_pointers_are_aligned_to_their_element_and_nothing_wider(dtype):
    size = np.dtype(dtype).itemsize
    k = V.pad_elements(size)
    assert k % 2 == 1 and k * size >= 64 and (k - 2) * size < 64
    for shape in SHAPES + ((257,),):
        v = V.View(np.zeros(shape, dtype), "offset", 0xFF, "cpu")
        assert v.form == "offset" and v.arg.is_contiguous() and v.arg.data_ptr() % (2 * size) == size
        assert v.arg.data_ptr() - v.buf.data_ptr() == k * size and v.total == v.arg.numel() + 2 * k
        if size == 1:
            assert v.arg.data_ptr() % 2 == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_layout_stays_inside_its_buffer(shape, dtype):
    """as many cells as the view has, from its first element, end before the buffer does - from the sizes, and again from
    the addresses of the views that are built"""
    a = raster(shape, dtype)
    n = a.size
    for layout in V.LAYOUTS:
        idx, total, form = V.cells_of(shape, a.itemsize, layout)
        assert 0 <= idx.reshape(-1)[0] and idx.reshape(-1)[0] + n <= total and idx.max() < total
        for poison in V.POISONS:
            v = V.View(a, layout, poison, "cpu")
            assert v.form == form and v.damaged() == 0 and np.array_equal(v.cells(), a)
            host = isinstance(v.arg, np.ndarray)
            start = v.arg.__array_interface__["data"][0] if host else v.arg.data_ptr()
            base = v.buf.__array_interface__["data"][0] if host else v.buf.data_ptr()
            assert base <= start and start + n * a.itemsize <= base + total * a.itemsize, (layout, shape)
            raw = (v.buf if host else v.buf.numpy()).reshape(-1).view(np.uint8).reshape(total, a.itemsize)
            outside = np.ones(total, bool)
            outside[idx.reshape(-1)] = False
            assert (raw[outside] == poison).all()
            if layout == "readonly":
                assert not v.arg.flags.writeable


def test_strided_views_are_not_contiguous_where_the_shape_allows_it():
    for shape, form in (((67, 131), "strided"), ((65, 1), "strided"), ((1, 65), "offset"), ((1, 1), "offset"),
                        ((257,), "strided"), ((1,), "offset"), ((257, 2), "strided"), ((256, 256, 4), "strided")):
        v = V.View(np.zeros(shape, np.float32), "strided", 0x5A, "cpu")
        assert v.form == form and v.arg.is_contiguous() == (form == "offset"), shape
    r = V.View(np.zeros((67, 131)), "strided", 0x5A, "cpu")
    assert tuple(r.buf.shape) == (69, 134) and r.arg.storage_offset() == 134 + 2 and r.arg.stride() == (134, 1)
    c = V.View(np.zeros((257, 3)), "strided", 0x5A, "cpu")
    assert tuple(c.buf.shape) == (259, 5) and c.arg.storage_offset() == 5 + 1
    t = V.View(np.zeros((256, 256, 3), np.uint8), "strided", 0x5A, "cpu")
    assert tuple(t.buf.shape) == (256, 256, 4) and t.arg.storage_offset() == 0
    x = V.View(np.zeros(257), "strided", 0x5A, "cpu")
    assert tuple(x.buf.shape) == (515,) and x.arg.stride() == (2,) and x.arg.storage_offset() == 1
    tr = V.View(raster(), "transposed", 0x5A, "cpu")
    assert tr.arg.stride() == (1, 67) and not tr.arg.is_contiguous()


def test_host_layouts_are_what_numpy_makes():
    a = raster()
    f = V.View(a, "fortran", 0xFF, "cpu").arg
    assert f.flags.f_contiguous and f.strides == np.asfortranarray(a).strides and np.array_equal(f, a)
    r = V.View(a, "reversed", 0xFF, "cpu").arg
    assert r.strides == a[::-1, ::-1].strides and np.array_equal(r, a)
    x = V.View(a[0], "reversed", 0xFF, "cpu").arg
    assert x.strides == (-8,) and np.array_equal(x, a[0])
    ro = V.View(a, "readonly", 0xFF, "cpu").arg
    assert ro.flags.c_contiguous and not ro.flags.writeable and np.array_equal(ro, a)
    assert V.layouts_for([a[0]]) == ["offset", "strided", "reversed", "readonly"]
    assert V.layouts_for([a[0], a], fills=True) == ["offset", "strided", "transposed", "fortran", "reversed"]
    assert V.layouts_for([]) == []
