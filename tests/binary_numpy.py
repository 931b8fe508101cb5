"""The contract of neilpy_amd/binary.py restated in NumPy (a plain helper module, no test in it, and no import of the
package): members about a centre, erosion as an AND and dilation as an OR of shifted reads with a
border value, the masked step and its repetition, opening, closing, hit-or-miss, propagation, fill_holes, and the
propagation identity through the components of the mask.  tests/test_binary_host.py pins it to scipy.ndimage."""
import numpy as np

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)


def origin_pair(origin):
    return tuple(origin) if hasattr(origin, "__iter__") else (origin, origin)


def origin_range(n):
    """the origins accepted for a structure axis of length n"""
    return range(-(n // 2), (n - 1) // 2 + 1)


def origins_of(shape):
    return [(a, b) for a in origin_range(shape[0]) for b in origin_range(shape[1])]


def members(structure, origin=0):
    """(dr, dc) = member - centre for every member, the centre at size // 2 + origin per axis, in C order"""
    s = CROSS if structure is None else np.asarray(structure).astype(bool)
    o = origin_pair(origin)
    for n, v in zip(s.shape, o):
        if v not in origin_range(n):
            raise ValueError("origin outside the accepted range")
    cr, cc = s.shape[0] // 2 + o[0], s.shape[1] // 2 + o[1]
    return [(int(r) - cr, int(c) - cc) for r, c in zip(*np.nonzero(s))]


def centre_is_member(structure, origin=0):
    return (0, 0) in members(structure, origin)


def shifted(S, dr, dc, border):
    """out[p] = S[p + (dr, dc)], cells outside the raster read as ``border``"""
    rows, cols = S.shape
    out = np.full(S.shape, bool(border))
    r0, r1 = max(0, -dr), min(rows, rows - dr)
    c0, c1 = max(0, -dc), min(cols, cols - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = S[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def erode_once(S, offs, border):
    out = np.ones(S.shape, bool)
    for dr, dc in offs:
        out &= shifted(S, dr, dc, border)
    return out


def dilate_once(S, offs, border):
    out = np.zeros(S.shape, bool)
    for dr, dc in offs:
        out |= shifted(S, -dr, -dc, border)
    return out


def _run(input, structure, iterations, mask, border_value, origin, once):
    S = np.asarray(input) != 0
    offs = members(structure, origin)
    if iterations < 1 and (0, 0) not in offs:
        raise NotImplementedError("iterations < 1 needs the centre to be a member")
    M = None if mask is None else np.asarray(mask) != 0
    k = 0
    while iterations < 1 or k < iterations:
        new = once(S, offs, border_value)
        if M is not None:
            new = np.where(M, new, S)
        k += 1
        if np.array_equal(new, S):
            break                                   # a step that changes nothing: every later one changes nothing
        S = new
    return S


def binary_erosion(input, structure=None, iterations=1, mask=None, border_value=0, origin=0):
    return _run(input, structure, iterations, mask, border_value, origin, erode_once)


def binary_dilation(input, structure=None, iterations=1, mask=None, border_value=0, origin=0):
    return _run(input, structure, iterations, mask, border_value, origin, dilate_once)


def binary_opening(input, structure=None, iterations=1, origin=0, mask=None, border_value=0):
    return binary_dilation(binary_erosion(input, structure, iterations, mask, border_value, origin), structure, iterations, mask,
                           border_value, origin)


def binary_closing(input, structure=None, iterations=1, origin=0, mask=None, border_value=0):
    return binary_erosion(binary_dilation(input, structure, iterations, mask, border_value, origin), structure, iterations, mask,
                          border_value, origin)


def binary_hit_or_miss(input, structure1=None, structure2=None, origin1=0, origin2=None):
    S = np.asarray(input) != 0
    s1 = CROSS if structure1 is None else np.asarray(structure1).astype(bool)
    s2 = ~s1 if structure2 is None else np.asarray(structure2).astype(bool)
    o2 = origin1 if origin2 is None else origin2
    return erode_once(S, members(s1, origin1), 0) & erode_once(~S, members(s2, o2), 1)


def binary_propagation(input, structure=None, mask=None, border_value=0, origin=0):
    return binary_dilation(input, structure, -1, mask, border_value, origin)


def binary_fill_holes(input, structure=None, origin=0):
    S = np.asarray(input) != 0
    return ~binary_dilation(np.zeros(S.shape, bool), structure, -1, ~S, 1, origin)


# ------------------------------------------------------------------------------------------
# the propagation identity: the converged result from the components of the mask
# ------------------------------------------------------------------------------------------
def propagation_by_labels(input, structure, mask, border_value, label):
    """binary_propagation for a centrally symmetric 3 x 3 structure with its centre set, without iterating.  ``label`` is
    a labelling function ``(mask, structure) -> (labels, n)``.  S1 = one masked dilation step of the input (it brings in
    the border value and the set cells outside the mask); inside the mask a cell is set iff its component of the mask
    holds a cell of S1, outside it keeps its value."""
    S = np.asarray(input) != 0
    M = np.ones(S.shape, bool) if mask is None else np.asarray(mask) != 0
    s = CROSS if structure is None else np.asarray(structure).astype(bool)
    assert s.shape == (3, 3) and s[1, 1] and np.array_equal(s, s[::-1, ::-1])
    S1 = np.where(M, dilate_once(S, members(s), border_value), S)
    L, n = label(M, s)
    flag = np.zeros(n + 1, bool)
    flag[L[S1 & M]] = True
    return np.where(M, flag[L], S)


def fill_holes_by_labels(input, structure, label):
    S = np.asarray(input) != 0
    return ~propagation_by_labels(np.zeros(S.shape, bool), structure, ~S, 1, label)
