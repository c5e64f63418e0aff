"""Case table of tests/test_gpu_complex_taps.py: FIRFilter shapes with COMPLEX taps on the boundaries of the complex register-tap predicate
(csrc/fir_creg.hip, fir_creg_ok), each with the kernel path mdsp_fir_kernel_path must report: 1 the complex register-tap kernel, 0 the generic
kernel.  The paths were read off the predicate; the trailing comment names the residues per thread P the launch takes.

The predicate: taps per phase tp = ceil(hlen / L) rounded up to a window TPC (steps of 8 to 64, then 80, 96, 112), L <= 1024, and the tap registers
P (TPC + P - 1) 2 (bytes of the arithmetic / 4) within the budget -- 230 at <= 256 phase groups (170 for two residues over a ComplexF64 window), 96 at
257 .. 1024 groups with P = 1 (48 over a ComplexF64 window); two residues per thread need M <= L and at most 256 groups.  Largest tp per case:

                                          P = 1, <= 256 groups   P = 2, <= 256 groups   P = 1, <= 1024 groups
    Float32 arithmetic                          112                     56                     48
    Float64 arithmetic, real signal              56                     24                     24
    Float64 arithmetic, complex signal           56                     16                      8

and the smallest tile -- max(1, 256 / groups) rounds of M samples plus the window, in the signal's own class -- must fit 150 KiB of LDS (decimators:
ComplexF64 up to M = 37, ComplexF32 up to 74, Float32 up to 149).  mdsp_fir_set_exact takes the generic kernel.  The arithmetic is Float64 whenever taps
or signal are double precision.

Row: (L, M, hlen, taps dtype, signal dtype, knobs, taps, expected path)
  knobs: (("exact", 1),) calls mdsp_fir_set_exact(f, 1)
  taps:  "rand" (seeded complex normal taps) or "rsf" (oracle.design.resample_filter(L // M) shifted to a channel centre: h[k] cis(2 pi 0.1 k / L))

Per dtype pair: both sides of the TPC edge at one residue per thread (3//8), both sides of the two-residue edge (5//3: P = 2, then P = 1), L = 256 / 257
and 512 / 513 just past the two-residue window, the 1024-thread form at its TPC edge and L = 1025.  Then the kinds -- standard (1//1), interpolators,
decimators (the channelizer shape 1//8 with 8 x 37 taps is 296 taps per phase: generic), the tile edges of the decimators, the rational resampling
shapes with resample_filter-length banks -- and four rows with mdsp_fir_set_exact.
"""

CASES = [
    (3, 8, 336, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (3, 8, 337, 'c32', 'f32', (), 'rand', 0),
    (5, 3, 280, 'c32', 'f32', (), 'rand', 1),   # P = 2
    (5, 3, 281, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (256, 1, 14592, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (257, 1, 14649, 'c32', 'f32', (), 'rand', 0),
    (1024, 1025, 49152, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (1024, 1025, 49153, 'c32', 'f32', (), 'rand', 0),
    (1025, 1024, 2050, 'c32', 'f32', (), 'rand', 0),
    (512, 511, 24576, 'c32', 'f32', (), 'rand', 1),   # P = 2
    (513, 512, 25137, 'c32', 'f32', (), 'rand', 0),
    (3, 8, 168, 'c32', 'f64', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c32', 'f64', (), 'rand', 0),
    (5, 3, 120, 'c32', 'f64', (), 'rand', 1),   # P = 2
    (5, 3, 121, 'c32', 'f64', (), 'rand', 1),   # P = 1
    (256, 1, 6400, 'c32', 'f64', (), 'rand', 1),   # P = 1
    (257, 1, 6425, 'c32', 'f64', (), 'rand', 0),
    (1024, 1025, 24576, 'c32', 'f64', (), 'rand', 1),   # P = 1
    (1024, 1025, 24577, 'c32', 'f64', (), 'rand', 0),
    (1025, 1024, 2050, 'c32', 'f64', (), 'rand', 0),
    (512, 511, 12288, 'c32', 'f64', (), 'rand', 1),   # P = 2
    (513, 512, 12825, 'c32', 'f64', (), 'rand', 0),
    (3, 8, 336, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (3, 8, 337, 'c32', 'c32', (), 'rand', 0),
    (5, 3, 280, 'c32', 'c32', (), 'rand', 1),   # P = 2
    (5, 3, 281, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (256, 1, 14592, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (257, 1, 14649, 'c32', 'c32', (), 'rand', 0),
    (1024, 1025, 49152, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (1024, 1025, 49153, 'c32', 'c32', (), 'rand', 0),
    (1025, 1024, 2050, 'c32', 'c32', (), 'rand', 0),
    (512, 511, 24576, 'c32', 'c32', (), 'rand', 1),   # P = 2
    (513, 512, 25137, 'c32', 'c32', (), 'rand', 0),
    (3, 8, 168, 'c32', 'c64', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c32', 'c64', (), 'rand', 0),
    (5, 3, 80, 'c32', 'c64', (), 'rand', 1),   # P = 2
    (5, 3, 81, 'c32', 'c64', (), 'rand', 1),   # P = 1
    (256, 1, 4352, 'c32', 'c64', (), 'rand', 1),   # P = 1
    (257, 1, 4369, 'c32', 'c64', (), 'rand', 0),
    (1024, 1025, 8192, 'c32', 'c64', (), 'rand', 1),   # P = 1
    (1024, 1025, 8193, 'c32', 'c64', (), 'rand', 0),
    (1025, 1024, 2050, 'c32', 'c64', (), 'rand', 0),
    (512, 511, 4096, 'c32', 'c64', (), 'rand', 1),   # P = 2
    (513, 512, 4617, 'c32', 'c64', (), 'rand', 0),
    (3, 8, 168, 'c64', 'f32', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c64', 'f32', (), 'rand', 0),
    (5, 3, 120, 'c64', 'f32', (), 'rand', 1),   # P = 2
    (5, 3, 121, 'c64', 'f32', (), 'rand', 1),   # P = 1
    (256, 1, 6400, 'c64', 'f32', (), 'rand', 1),   # P = 1
    (257, 1, 6425, 'c64', 'f32', (), 'rand', 0),
    (1024, 1025, 24576, 'c64', 'f32', (), 'rand', 1),   # P = 1
    (1024, 1025, 24577, 'c64', 'f32', (), 'rand', 0),
    (1025, 1024, 2050, 'c64', 'f32', (), 'rand', 0),
    (512, 511, 12288, 'c64', 'f32', (), 'rand', 1),   # P = 2
    (513, 512, 12825, 'c64', 'f32', (), 'rand', 0),
    (3, 8, 168, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c64', 'f64', (), 'rand', 0),
    (5, 3, 120, 'c64', 'f64', (), 'rand', 1),   # P = 2
    (5, 3, 121, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (256, 1, 6400, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (257, 1, 6425, 'c64', 'f64', (), 'rand', 0),
    (1024, 1025, 24576, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (1024, 1025, 24577, 'c64', 'f64', (), 'rand', 0),
    (1025, 1024, 2050, 'c64', 'f64', (), 'rand', 0),
    (512, 511, 12288, 'c64', 'f64', (), 'rand', 1),   # P = 2
    (513, 512, 12825, 'c64', 'f64', (), 'rand', 0),
    (3, 8, 168, 'c64', 'c32', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c64', 'c32', (), 'rand', 0),
    (5, 3, 80, 'c64', 'c32', (), 'rand', 1),   # P = 2
    (5, 3, 81, 'c64', 'c32', (), 'rand', 1),   # P = 1
    (256, 1, 4352, 'c64', 'c32', (), 'rand', 1),   # P = 1
    (257, 1, 4369, 'c64', 'c32', (), 'rand', 0),
    (1024, 1025, 8192, 'c64', 'c32', (), 'rand', 1),   # P = 1
    (1024, 1025, 8193, 'c64', 'c32', (), 'rand', 0),
    (1025, 1024, 2050, 'c64', 'c32', (), 'rand', 0),
    (512, 511, 4096, 'c64', 'c32', (), 'rand', 1),   # P = 2
    (513, 512, 4617, 'c64', 'c32', (), 'rand', 0),
    (3, 8, 168, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (3, 8, 169, 'c64', 'c64', (), 'rand', 0),
    (5, 3, 80, 'c64', 'c64', (), 'rand', 1),   # P = 2
    (5, 3, 81, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (256, 1, 4352, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (257, 1, 4369, 'c64', 'c64', (), 'rand', 0),
    (1024, 1025, 8192, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (1024, 1025, 8193, 'c64', 'c64', (), 'rand', 0),
    (1025, 1024, 2050, 'c64', 'c64', (), 'rand', 0),
    (512, 511, 4096, 'c64', 'c64', (), 'rand', 1),   # P = 2
    (513, 512, 4617, 'c64', 'c64', (), 'rand', 0),
    (1, 1, 7, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (1, 1, 66, 'c64', 'c64', (), 'rand', 0),
    (1, 1, 112, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (1, 1, 113, 'c32', 'f32', (), 'rand', 0),
    (1, 1, 56, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (1, 1, 57, 'c64', 'f32', (), 'rand', 0),
    (4, 1, 36, 'c32', 'c32', (), 'rand', 1),   # P = 2
    (7, 1, 50, 'c64', 'c64', (), 'rand', 1),   # P = 2
    (2, 1, 60, 'c32', 'f64', (), 'rand', 1),   # P = 1
    (1, 8, 296, 'c32', 'c32', (), 'rand', 0),
    (1, 8, 296, 'c64', 'c64', (), 'rand', 0),
    (1, 8, 296, 'c32', 'f32', (), 'rand', 0),
    (1, 4, 37, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (1, 4, 37, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (1, 3, 100, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (1, 2, 56, 'c64', 'f64', (), 'rand', 1),   # P = 1
    (1, 63, 50, 'c32', 'c64', (), 'rand', 0),
    (1, 37, 40, 'c64', 'c64', (), 'rand', 1),   # P = 1
    (1, 38, 40, 'c64', 'c64', (), 'rand', 0),
    (1, 74, 40, 'c32', 'c32', (), 'rand', 1),   # P = 1
    (1, 75, 40, 'c32', 'c32', (), 'rand', 0),
    (1, 149, 96, 'c32', 'f32', (), 'rand', 1),   # P = 1
    (1, 150, 96, 'c32', 'f32', (), 'rand', 0),
    (160, 147, 5921, 'c32', 'c32', (), 'rsf', 1),   # P = 2
    (160, 147, 5921, 'c64', 'c64', (), 'rsf', 1),   # P = 1
    (160, 147, 5921, 'c32', 'f32', (), 'rsf', 1),   # P = 2
    (160, 147, 5921, 'c64', 'f32', (), 'rsf', 1),   # P = 1
    (147, 160, 5881, 'c32', 'c32', (), 'rsf', 1),   # P = 1
    (147, 160, 5881, 'c64', 'c64', (), 'rsf', 1),   # P = 1
    (147, 160, 5881, 'c32', 'f32', (), 'rsf', 1),   # P = 1
    (147, 160, 5881, 'c64', 'f32', (), 'rsf', 1),   # P = 1
    (441, 160, 16317, 'c32', 'c32', (), 'rsf', 1),   # P = 2
    (441, 160, 16317, 'c64', 'c64', (), 'rsf', 0),
    (441, 160, 16317, 'c32', 'f32', (), 'rsf', 1),   # P = 2
    (441, 160, 16317, 'c64', 'f32', (), 'rsf', 0),
    (3, 8, 295, 'c32', 'c32', (), 'rsf', 1),   # P = 1
    (3, 8, 295, 'c64', 'c64', (), 'rsf', 0),
    (3, 8, 295, 'c32', 'f32', (), 'rsf', 1),   # P = 1
    (3, 8, 295, 'c64', 'f32', (), 'rsf', 0),
    (5, 3, 100, 'c32', 'c32', (('exact', 1),), 'rand', 0),
    (1, 4, 37, 'c64', 'c64', (('exact', 1),), 'rand', 0),
    (160, 147, 5921, 'c32', 'f32', (('exact', 1),), 'rsf', 0),
    (3, 2, 60, 'c64', 'f64', (('exact', 1),), 'rand', 0),
]
