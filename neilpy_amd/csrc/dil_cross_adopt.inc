// Per-radius adoption of the cross on load (morph_ring.h, ring_cross_kernel) in progressive_filter's default routing
// (SMRF_DIL_CROSS=1), fp32.  Index = radius; 1 = window R (after a two-pass window R - 1) launches no erosion: its dilation pass
// takes the 5-point cross of e_{R-1} while it loads it.  Only the radii with an empty leftover set P_R have an instance
// (smrf_dil_cross_has: 16, 21, 36).
// The rule (profiles/dil_cross.md): measured on MI355X, 16384^2, windows 1..50, this build with SMRF_DIL_CROSS=2 against the build
// before it, both interleaved in one process:
//     SMRF_DIL_CROSS=2 python tools/window_ab.py --libs parent.so --windows 50 --reps 5
// A radius is taken where its whole window is at least 3 percent faster; 36 only if the pair 36 + 37 is, because window 37
// loses its incremental erosion to the fold (smrf_pf_fold, kPfFoldAfter).  16: 1.087 -> 0.798 ms (-27 percent), 21: 1.123 ->
// 0.907 ms (-19 percent); 36: 1.362 -> 1.278 ms, but 36 + 37: 2.941 -> 2.996 ms, not taken.
// (Included inside namespace smrf.)
inline constexpr unsigned char kDilCrossAdoptF32[65] = {
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1,
    0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
