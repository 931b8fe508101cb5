// Per-radius adoption of the incremental erosion (morph_incero.h) in progressive_filter's default routing (SMRF_ERO_INC=1), fp32.
// Index = radius; 1 = window R (after a two-pass window R - 1) takes inc_erode_kernel instead of the ring erosion.
// Measured on MI355X, 16384^2, windows 1..50, SMRF_ERO_INC=2 against the build before it, both interleaved in one process
// with tools/window_ab.py (profiles/r06_ero_inc.md, profiles/r06_logs/window_ab_16384.log): a radius is taken where its
// window is at least 3 percent faster - 17 of the 35 radii 16..50, -2.97 ms of a 65.9 ms call.  The cost of the pass follows
// |P_R|: the radii with few leftover cells win by 12-23 percent (36, 38, 41, 46), those with 32 and more lose (32, 35, 37, 39),
// and below R = 28 the ring erosion is already as fast as the three plane touches of this pass (only R = 21, empty P_R, wins).
// R = 51..64 are not measured (the benchmark stops at 50) and stay on the ring erosion.  (Included inside namespace smrf.)
inline constexpr unsigned char kEroIncAdoptF32[65] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0,
    1, 0, 1, 0, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
