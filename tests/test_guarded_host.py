"""The guard-band harness (tests/guarded.py) proves itself on the CPU: small stand-in "kernels", plain torch code that
writes through a raw view of the arena, misbehave in each of the ways the harness is there to detect, and every check
fails when it should and passes when it should.  The stand-ins allocate through the ``torch`` module at call time, as
the package does."""
import numpy as np
import pytest
import torch

import guarded as G
from guarded import GuardError, guarded, same_bits


def kernel(x, bug=None, dtype=None):
    """out[i] = 2 * x[i] through a workspace cell per element, as a device kernel would address memory: base pointer
    plus index, nothing in the way of a stray one"""
    n = x.numel()
    out = torch.empty(x.shape, dtype=dtype or x.dtype, device=x.device)
    ws = torch.empty(n, dtype=torch.float64, device=x.device)
    g = G._active[0]
    cells, o0 = g.raw(out)
    wcells, w0 = g.raw(ws)
    xcells, x0 = g.raw(x)
    for i in range(n):
        if not (bug == "scratch" and i == 2):
            wcells[w0 + i] = float(xcells[x0 + i])          # the workspace cell is written before it is read ...
        if bug == "skip" and i == n - 1:
            continue                                        # ... a store that never happens
        cells[o0 + i] = 2 * wcells[w0 + i]
    if bug == "overrun":
        cells[o0 + n] = 7
    if bug == "underrun":
        cells[o0 - 1] = 7
    if bug == "inplace":
        xcells[x0 + 1] = xcells[x0 + 1] + 1
    return out


X = np.array([1.5, -2.0, 3.25, 0.0, 9.0])


def run(bug, poison, x=X, dtype=None):
    with guarded("cpu", poison) as g:
        xt = g.tensor(x)
        out = kernel(xt, bug, dtype)
    return g, xt, out


def test_a_correct_kernel_passes_every_check():
    outs = []
    for poison in G.POISONS:
        g, xt, out = run(None, poison)
        g.check()
        assert g.owns(out) and g.owns(xt) and g.unchanged(xt)
        assert np.array_equal(out.numpy(), 2 * X)
        outs.append(out.numpy())
    assert same_bits(*outs)


def test_layout_of_an_arena():
    with guarded("cpu", 0x5A) as g:
        e = torch.empty((3, 5), dtype=torch.float32)
        z = torch.zeros(7, dtype=torch.int64, device="cpu")
        o = torch.ones((2, 2), dtype=torch.uint8)
        f = torch.full((3,), 2.5, dtype=torch.float64)
        el = torch.empty_like(z)
        zl = torch.zeros_like(e, dtype=torch.float64)
        b = g.bytes_of(13)
    assert e.shape == (3, 5) and e.dtype == torch.float32 and e.is_contiguous()
    assert np.all(e.numpy().view(np.uint8) == 0x5A) and np.all(el.numpy().view(np.uint8) == 0x5A)     # empty: still poisoned
    assert np.all(b.numpy() == 0x5A) and b.numel() == 13
    assert torch.all(z == 0) and torch.all(o == 1) and torch.all(f == 2.5) and torch.all(zl == 0)
    assert zl.shape == e.shape and zl.dtype == torch.float64 and el.dtype == torch.int64
    for t in (e, z, o, f, el, zl, b):
        assert g.owns(t)
        a = g._arena_of(t)
        nbytes = t.numel() * t.element_size()
        assert a.buf.numel() == 2 * G.GUARD + nbytes                   # the tail guard starts at the exact last byte
        assert t.data_ptr() - a.buf.data_ptr() == G.GUARD and G.GUARD % 512 == 0
        raw = a.buf.numpy()
        assert np.all(raw[:G.GUARD] == 0x5A) and np.all(raw[G.GUARD + nbytes:] == 0x5A)      # fills stay inside
    assert len(g.arenas) == 7
    g.check()


def test_requests_that_pass_through():
    with guarded("cpu", 0xFF) as g:
        nothing = torch.empty(0, dtype=torch.uint8)
        none2d = torch.zeros((0, 5))
        elsewhere = torch.empty(4, device="meta")
        into = torch.zeros(3)
        n = len(g.arenas)
        same = torch.empty(3, out=into)
        assert len(g.arenas) == n == 1 and same.data_ptr() == into.data_ptr()
    assert not g.owns(nothing) and not g.owns(none2d) and not g.owns(elsewhere)
    assert none2d.shape == (0, 5) and elsewhere.device.type == "meta"


def test_names_are_restored_also_after_an_exception():
    before = {name: getattr(torch, name) for name in G.PATCHED}
    with pytest.raises(ZeroDivisionError):
        with guarded("cpu", 0xFF):
            assert all(getattr(torch, name) is not before[name] for name in G.PATCHED)
            1 / 0
    assert all(getattr(torch, name) is before[name] for name in G.PATCHED)
    with guarded("cpu", 0xFF):
        pass
    assert all(getattr(torch, name) is before[name] for name in G.PATCHED) and not G._active


@pytest.mark.parametrize("poison", G.POISONS)
def test_a_write_one_element_past_the_end(poison):
    g, xt, out = run("overrun", poison)
    assert np.array_equal(out.numpy(), 2 * X)                    # invisible in the returned array
    with pytest.raises(GuardError) as e:
        g.check()
    msg = str(e.value)
    assert "behind float64(5,)" in msg and "test_guarded_host.py" in msg, msg
    assert "8 guard byte(s)" in msg and "first at byte offset +0 from the interior's end" in msg, msg


@pytest.mark.parametrize("poison", G.POISONS)
def test_a_write_one_element_before_the_start(poison):
    g, xt, out = run("underrun", poison, X.astype(np.float32))
    assert np.array_equal(out.numpy(), 2 * X)
    with pytest.raises(GuardError) as e:
        g.check()
    msg = str(e.value)
    assert "in front of float32(5,)" in msg and "test_guarded_host.py" in msg, msg
    assert "first at byte offset -4 from the interior's start" in msg, msg


def test_an_unwritten_output_cell():
    a, b = (run("skip", p)[2].numpy() for p in G.POISONS)
    assert not same_bits(a, b)
    assert np.isnan(a[-1]) and np.array_equal(a[:-1], b[:-1])
    good = [run(None, p)[2].numpy() for p in G.POISONS]
    assert same_bits(*good)


def test_an_unwritten_uint8_cell_whose_right_value_is_a_poison_byte():
    """255 is the right answer and the 0xFF poison: that run alone looks right, the pair does not"""
    x = np.array([3.0, 100.0, 127.5])
    a, b = (run("skip", p, x, torch.uint8)[2].numpy() for p in G.POISONS)
    want = np.array([6, 200, 255], np.uint8)
    assert np.array_equal(a, want) and not np.array_equal(b, want) and not same_bits(a, b)
    good = [run(None, p, x, torch.uint8)[2].numpy() for p in G.POISONS]
    assert same_bits(*good) and np.array_equal(good[0], want)
    # and the mirror image: 0x5A = 90 is the right answer
    x = np.array([3.0, 100.0, 45.0])
    a, b = (run("skip", p, x, torch.uint8)[2].numpy() for p in G.POISONS)
    assert np.array_equal(b, np.array([6, 200, 90], np.uint8)) and not same_bits(a, b)


def test_a_result_that_depends_on_an_uninitialised_workspace_cell():
    a, b = (run("scratch", p)[2].numpy() for p in G.POISONS)
    assert not same_bits(a, b) and np.array_equal(np.delete(a, 2), np.delete(b, 2))
    for p in G.POISONS:
        g = run("scratch", p)[0]
        g.check()                                               # no guard is touched: only the pair shows it


def test_an_input_modified_in_place():
    g, xt, out = run("inplace", 0xFF)
    g.check()
    assert not g.unchanged(xt)
    assert g.unchanged(xt, where=np.array([1, 0, 1, 1, 1], bool))           # the other cells kept their bits
    assert not g.unchanged(xt, where=np.array([0, 1, 0, 0, 0], bool))


def test_unchanged_compares_bits_not_values():
    payload = np.array([0x7FF8000000000001, 0x7FF8000000000002], np.uint64).view(np.float64)
    with guarded("cpu", 0xFF) as g:
        t = g.tensor(np.array([payload[0], 0.0, 1.0]))
        assert g.unchanged(t)
        t[0] = float("nan")                                     # another NaN: equal under equal_nan, not the same bits
        t.numpy().view(np.uint64)[0] = payload.view(np.uint64)[1]
        assert not g.unchanged(t)
        g.snapshot(t)
        assert g.unchanged(t)
        t[1] = -0.0                                             # -0.0 == 0.0
        assert not g.unchanged(t)


def test_a_tensor_allocated_behind_the_harness():
    with guarded("cpu", 0xFF) as g:
        xt = g.tensor(X)
        out = kernel(xt)
        copy = out.clone()                                      # a torch op allocates in C++, not through torch.empty
        view = out[1:3]
        host = torch.from_numpy(X.copy())
    assert g.owns(out) and g.owns(view) and not g.owns(copy) and not g.owns(host) and not g.owns(X)
    with guarded("cpu", 0xFF) as g2:
        pass
    assert not g2.owns(out)                                     # another harness's arena is not this one's


def test_every_export_is_guarded_left_out_with_a_reason_or_launches_nothing():
    """tests/family_cases.py classifies every public name of the package: built into cases that run under the harness, left
    out with a reason, or launching no kernel.  A family added later cannot go unguarded silently: its names are in none of
    the lists, and a name of GUARDED without a builder fails here."""
    import re
    import types
    import neilpy_amd
    import family_cases as T
    exports = {n for n, v in vars(neilpy_amd).items() if not n.startswith("_") and not isinstance(v, types.ModuleType)}
    lists = (set(T.GUARDED), set(T.LEFT_OUT), set(T.NO_KERNEL))
    assert len(T.GUARDED) == len(lists[0]) and len(T.NO_KERNEL) == len(lists[2])
    assert not (lists[0] & lists[1]) and not (lists[0] & lists[2]) and not (lists[1] & lists[2])
    assert lists[0] | lists[1] | lists[2] == exports, (sorted(exports - lists[0] - lists[1] - lists[2]),
                                                        sorted((lists[0] | lists[1] | lists[2]) - exports))
    assert all(isinstance(r, str) and r for r in T.LEFT_OUT.values())
    assert set(T.BUILDERS) == lists[0], sorted(set(T.BUILDERS) ^ lists[0])
    # every guarded name is really called: as the literal F("name"), or as F(fn) over one of the four tuples
    src = open(T.__file__.rstrip("c")).read()
    called = set(re.findall(r'\bF\("(\w+)"\)', src)) | set(T.SURFACE) | set(T.TERRAIN) | set(T.DISK) | set(T.MORPHOLOGY)
    assert "F(fn)" in src
    assert called == lists[0], sorted(lists[0] ^ called)
    assert all(isinstance(r, str) and r for r in T.NOT_OWNED.values())
