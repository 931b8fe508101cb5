// Per-radius adoption of the incremental erosion (morph_incero.h) in progressive_filter's default routing (SMRF_ERO_INC=1), fp32.
// Index = radius; 1 = window R (after a two-pass window R - 1) takes inc_erode_kernel instead of the ring erosion.
// Measured on MI355X, 16384^2, windows 1..50, this build with SMRF_ERO_INC=2 against the build before it with SMRF_ERO_INC=0
// (every window on the ring erosion), both interleaved in one process:
//     SMRF_ERO_INC=2 python tools/window_ab.py --libs parent.so --libs-env SMRF_ERO_INC=0 --windows 50 --reps 5
// (profiles/incero_mirror.md section 3, profiles/incero_mirror_logs/window_ring_ab.log).  A radius is taken where its whole
// window is at least 3 percent faster - 23 of the 35 radii 16..50: 21, 28, 29 and every radius from 31 up.  With the mirror
// plan and a third wave per SIMD the pass costs 0.62-0.67 ms (its three plane touches) up to 36 cells and at most 0.71 ms
// at 48, so 32, 33, 34, 35, 37 and 39 now win 5-12 percent of the window (they were 2.2-2.9 percent short, 32 lost).  24 and 30
// met the rule in this measurement (-3.2 and -4.7 percent) but not in the one of an earlier session with the same kernels
// (-1.5 and -2.2) and stay on the ring erosion; below R = 28 the ring erosion itself runs at the three-plane-touch time (only
// R = 21, empty P_R, wins).  R = 51..64 are not measured (the benchmark stops at 50) and stay on the ring erosion.
// (Included inside namespace smrf.)
inline constexpr unsigned char kEroIncAdoptF32[65] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
