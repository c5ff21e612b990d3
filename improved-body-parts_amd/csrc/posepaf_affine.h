// posepaf_affine.h -- cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) sampling as OpenCV 3.4 (imgwarp.cpp) computes it, for the
// test-time rotation search (utils/parse_skeletons.py:214-218, :265-267).  The host inverts the matrix (posepaf/rotation.py,
// in double, as warpAffine does without WARP_INVERSE_MAP); the kernels receive the 6 inverted doubles.  For a destination
// pixel (x, y):
//     X = (rint((M1 y + M2) 1024) + 16 + rint(M0 x 1024)) >> 5,  Y likewise with M4, M5, M3   (AB_BITS 10, INTER_BITS 5)
//     sx = X >> 5, fx = X & 31;  weights (1 - fy/32)(1 - fx/32), (1 - fy/32) fx/32, fy/32 (1 - fx/32), fy/32 fx/32 (exact)
//     value = ((v00 w0 + v01 w1) + v10 w2) + v11 w3, taps outside the source read 0; a block wholly outside gives exactly 0.
// Every operation is rounded on its own (no contraction), like the restatement in tests/rotation_reference.py.
#ifndef POSEPAF_AFFINE_H
#define POSEPAF_AFFINE_H

#include <hip/hip_runtime.h>

namespace pp {

struct Affine6 {
    double m[6];   // inverted matrix, row-major: src = (m0 x + m1 y + m2, m3 x + m4 y + m5)
};

struct AffineTap {
    int sx, sy;    // top-left tap
    float w[4];    // weights of (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)
};

__device__ __forceinline__ void affine_src(const double *m, int x, int y, int &sx, int &sy, int &fx, int &fy) {
    const int adelta = __double2int_rn(__dmul_rn(__dmul_rn(m[0], (double)x), 1024.0));
    const int bdelta = __double2int_rn(__dmul_rn(__dmul_rn(m[3], (double)x), 1024.0));
    const int X0 = __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[1], (double)y), m[2]), 1024.0)) + 16;
    const int Y0 = __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[4], (double)y), m[5]), 1024.0)) + 16;
    const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    sx = X >> 5;
    sy = Y >> 5;
    fx = X & 31;
    fy = Y & 31;
}

// the row terms X0 / Y0 (rint((M1 y + M2) 1024) + 16, ...) and the column terms adelta / bdelta of OpenCV's tables
__device__ __forceinline__ int2 affine_row(const double *m, int y) {
    return make_int2(__double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[1], (double)y), m[2]), 1024.0)) + 16,
                     __double2int_rn(__dmul_rn(__dadd_rn(__dmul_rn(m[4], (double)y), m[5]), 1024.0)) + 16);
}
__device__ __forceinline__ int2 affine_col(const double *m, int x) {
    return make_int2(__double2int_rn(__dmul_rn(__dmul_rn(m[0], (double)x), 1024.0)),
                     __double2int_rn(__dmul_rn(__dmul_rn(m[3], (double)x), 1024.0)));
}

// the tap from a row term and a column term
__device__ __forceinline__ AffineTap affine_tap_rc(int2 row, int2 col) {
    AffineTap t;
    const int X = (row.x + col.x) >> 5, Y = (row.y + col.y) >> 5;
    t.sx = X >> 5;
    t.sy = Y >> 5;
    const float ax = (float)(X & 31) / 32.0f, ay = (float)(Y & 31) / 32.0f;
    const float bx = __fadd_rn(1.0f, -ax), by = __fadd_rn(1.0f, -ay);
    t.w[0] = __fmul_rn(by, bx);
    t.w[1] = __fmul_rn(by, ax);
    t.w[2] = __fmul_rn(ay, bx);
    t.w[3] = __fmul_rn(ay, ax);
    return t;
}

__device__ __forceinline__ AffineTap affine_tap(const double *m, int x, int y) {
    AffineTap t;
    int fx, fy;
    affine_src(m, x, y, t.sx, t.sy, fx, fy);
    const float ax = (float)fx / 32.0f, ay = (float)fy / 32.0f;
    const float bx = __fadd_rn(1.0f, -ax), by = __fadd_rn(1.0f, -ay);
    t.w[0] = __fmul_rn(by, bx);
    t.w[1] = __fmul_rn(by, ax);
    t.w[2] = __fmul_rn(ay, bx);
    t.w[3] = __fmul_rn(ay, ax);
    return t;
}

// true when all four taps lie outside an (h, w) source: the result is exactly 0 (BORDER_CONSTANT)
__device__ __forceinline__ bool affine_outside(const AffineTap &t, int h, int w) {
    return t.sx >= w || t.sx + 1 < 0 || t.sy >= h || t.sy + 1 < 0;
}

__device__ __forceinline__ float affine_combine(const AffineTap &t, float v0, float v1, float v2, float v3) {
    float v = __fadd_rn(__fmul_rn(v0, t.w[0]), __fmul_rn(v1, t.w[1]));
    v = __fadd_rn(v, __fmul_rn(v2, t.w[2]));
    return __fadd_rn(v, __fmul_rn(v3, t.w[3]));
}

}  // namespace pp

#endif
