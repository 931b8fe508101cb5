// Per-radius adoption of the incremental erosion (morph_incero.h) in progressive_filter's default routing (SMRF_ERO_INC=1), fp32.
// Index = radius; 1 = window R (after a two-pass window R - 1) takes inc_erode_kernel instead of the ring erosion.
// Measured on MI355X, 16384^2, windows 1..50, this build with SMRF_ERO_INC=2 against the build before it with SMRF_ERO_INC=0
// (every window on the ring erosion), both interleaved in one process:
//     SMRF_ERO_INC=2 python tools/window_ab.py --libs parent.so --libs-env SMRF_ERO_INC=0 --windows 50 --reps 5
// (profiles/incero_overlap.md section 3, profiles/incero_overlap_logs/window_ring_ab.log).  A radius is taken where its whole
// window is at least 3 percent faster - 17 of the 35 radii 16..50.  The pass costs 0.46 ms with an empty P_R, 0.63-0.66 ms (its
// three plane touches) with 8 cells and up to 0.86 ms at 48 cells; it wins 4-21 percent of the window at 21, 28, 29, 31, 36, 38
// and every radius from 40 up.  33, 34, 35 and 39 are 2.2-2.9 percent faster, short of the rule, 32 (32 cells against a fast
// ring erosion) loses 3 percent, and below R = 28 the ring erosion itself runs at the three-plane-touch time (only R = 21,
// empty P_R, wins).  R = 51..64 are not measured (the benchmark stops at 50) and stay on the ring erosion.
// (Included inside namespace smrf.)
inline constexpr unsigned char kEroIncAdoptF32[65] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0,
    0, 0, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
