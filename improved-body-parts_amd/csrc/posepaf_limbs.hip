// posepaf_limbs.hip -- the ellipse / alpha-blend skeleton drawing of the demo's original branch (reference demo_image.py:218-240)
// for a whole bucket in one launch, straight from pp_record[b] in device memory, BIT-EQUAL to the NumPy renderer
// utils/draw.py:draw_limbs_original on the persons and candidates the record stands for (posepaf/render.py:record_to_persons).
//
// Instances are drawn limb type after limb type (the 18 entries of DRAW_LIST), inside a type human after human; instance (t, h)
// exists when both joints (pa, pb) = LIMB_PAIRS[DRAW_LIST[t]] of human h are present.  With the coordinates widened to double,
//   dy = Y0 - Y1, dx = X0 - X1 (joint pa first);  length = sqrt(dy dy + dx dx);  a = max((double)(int)(length / 2), 0.5), b = 3;
//   k = int(degrees(atan2(dy, dx)))  (limb_angle_deg below: no libm);   (c, s) = (cos, sin)(k pi / 180) from the HOST's table;
//   rings   9 <= (x - rx)^2 + (y - ry)^2 <= 25  about (int(X0), int(Y0)) and (int(X1), int(Y1)), in integers, black;
//   ellipse about (cx, cy) = (int((X0 + X1) / 2), int((Y0 + Y1) / 2)), in float64, one rounding per operation:
//       u = (x - cx) c + (y - cy) s;  v = (-(x - cx)) s + (y - cy) c;  (u / a)(u / a) + (v / b)(v / b) <= 1.0,  LimbColors[board[t]].
// A pixel that one of the three tests hits becomes clip(rint(px 0.4 + cur 0.6), 0, 255) per channel (float64, ties to even) with
// cur = the ellipse colour where the ellipse hits (it is painted after the rings) and black otherwise; draw.py blends the WHOLE
// canvas per instance, but rint(c 0.4 + c 0.6) == c for every byte c (tests/test_draw_limbs_cpu.py), so a pixel nothing hits
// keeps its value and every pixel is the fold, in instance order, over the instances that hit it.  draw.py's bounding boxes cut
// no primitive (same test), so there is no box in the contract; the boxes below only cull.
//
// A workgroup takes one 64 x 16 tile of one image.  The up to 18 x 128 instances go through LDS 256 at a time IN DRAW ORDER:
// thread i of a chunk takes instance base + i, keeps it when its box (the rings' +-6 and the ellipse's +-(max(a, 3) + 1)) reaches
// the tile, and the kept ones are compacted in order (ballot + prefix over the four waves); then every thread folds the list
// FORWARDS over its four pixels.  Chunks are consumed in ascending order and each is finished before the next is listed, so the
// fold order across chunk boundaries is the draw order.  No atomics, no memset, no allocation, nothing shared between workgroups.
// Compiled with -ffp-contract=off (csrc/Makefile STRICT): products and sums round separately, the f64 division and square root
// are hipcc's correctly rounded ones.  Exact for coordinates within +-32767; beyond that the boxes are clipped in 64 bits and
// nothing outside the image's own pixels is ever written.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/posepaf.h"

namespace {

constexpr int LB_TW = 64, LB_TH = 16;        // tile: 16 threads x 4 pixels wide, 16 rows
constexpr int LB_THREADS = 256;              // = instances listed per chunk
constexpr int LB_TYPES = 18;                 // len(DRAW_LIST)
constexpr int LB_ANGLES = 361;               // k = -180 .. 180 at table[2 (k + 180)] = cos, [2 (k + 180) + 1] = sin

// LIMB_PAIRS[i] for i in DRAW_LIST = [0, 5 .. 20, 29] (posepaf/skeleton.py; config/config.py:116-121, :154)
__device__ const signed char d_limb_pairs[LB_TYPES][2] = {{1, 0},  {0, 14}, {0, 15}, {14, 16}, {15, 17}, {1, 2},   {2, 3},   {3, 4},   {1, 5},
                                                          {5, 6},  {6, 7},  {1, 8},  {8, 9},   {9, 10},  {1, 11},  {11, 12}, {12, 13}, {8, 11}};
// LimbColors[color_board[t]], color_board = [0, 5 .. 21] (utils/draw.py:18-21, :103), (B, G, R)
__device__ const unsigned char d_limb_colors[LB_TYPES][3] = {
    {128, 114, 250}, {255, 85, 0},  {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0},   {0, 255, 85},  {0, 255, 170},
    {0, 255, 255},   {0, 170, 255}, {0, 85, 255},  {0, 0, 255},   {85, 0, 255},  {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}};

// k = int(math.degrees(math.atan2(dy, dx))) (truncation towards zero, k in [-180, 180]) without a libm call, for finite dy, dx.
// `tab` is pp_limb_angle_table's table.
//  * The exact directions are branches: dy == 0 (0, or +-180 for a negative dx, -0.0 included), dx == 0 (+-90), |dy| == |dx|
//    (+-45, +-135); the sign of dy (of -0.0 too) is the sign of the result, as for atan2.
//  * Two slivers beside an axis belong to the axis: atan2 returns the double nearest pi (pi / 2) once the direction is within
//    2^-52 + (pi - (double)pi) = 3.445e-16 rad of the negative x axis (half of that of the y axis, from the right), and degrees()
//    of that double is 180.0 (90.0) exactly.  Coordinates reach them only with a joint distance below 1e-13 px across a limb,
//    but a float32 record can hold one.  (Beside 0 and beyond +-90 truncation gives the axis anyway.)
//  * Everywhere else the angle is no integer degree (tan of a non-multiple of 45 degrees is irrational, dy / dx is not), and k is
//    found by bisection over j on the sign of  dy cos(j) - dx sin(j) = r sin(angle - j)  with cos / sin from the table.  The
//    sign is safe because dy and dx are differences of float32 or int values: over 2e6 random such pairs the angle came no closer
//    to an integer degree than 3.6e-7 degrees (6e-9 rad), while the rounding of the two products, of their difference and of the
//    table's entries is about 1e-16 relative to r; Python's own value is off by about 1e-13 degrees at most.  Differences
//    that put the angle within 1e-12 degrees of an integer degree other than on the axes (joints 2^-50 px apart from a diagonal,
//    say) are outside the claim.
__host__ __device__ inline int limb_angle_deg(double dy, double dx, const double *tab) {
    if (!(dy == dy) || !(dx == dx)) return 0;
    const bool ny = __builtin_signbit(dy), nx = __builtin_signbit(dx);
    const double ay = ny ? -dy : dy, ax = nx ? -dx : dx;
    int k;
    if (ay == 0.0) {
        k = nx ? 180 : 0;
    } else if (ax == 0.0) {
        k = 90;
    } else if (ay == ax) {
        k = nx ? 135 : 45;
    } else if (nx && ay <= ax * 0x1.8d313198a2e03p-52) {
        k = 180;
    } else if (!nx && ax <= ay * 0x1.8d313198a2e03p-53) {
        k = 90;
    } else {
        int lo = 0, hi = 180;                 // 0 < angle < 180: sin(angle - lo) > 0 > sin(angle - hi) throughout
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            const double t0 = ay * tab[2 * (mid + 180)], t1 = dx * tab[2 * (mid + 180) + 1];
            if (t0 - t1 > 0.0)
                lo = mid;
            else
                hi = mid;
        }
        k = lo;
    }
    return ny ? -k : k;
}

// the table, filled by the C library at run time (a volatile factor keeps the compiler from folding the calls): the bits of
// math.cos(math.radians(k)) and math.sin(math.radians(k)), which evaluate k * (pi / 180) the same way
void fill_angle_table(double *tab) {
    volatile double deg_to_rad = M_PI / 180.0;
    for (int k = -180; k <= 180; k++) {
        const double r = (double)k * deg_to_rad;
        tab[2 * (k + 180)] = std::cos(r);
        tab[2 * (k + 180) + 1] = std::sin(r);
    }
}

const double *host_angle_table() {
    static const struct Table {
        double v[2 * LB_ANGLES];
        Table() { fill_angle_table(v); }
    } table;
    return table.v;
}

// a joint coordinate widened to double; false for a non-finite float32 (the instance is skipped: Python would raise there)
__device__ __forceinline__ bool coord_f64(int raw, bool is_float, double &out) {
    if (!is_float) {
        out = (double)raw;
        return true;
    }
    out = (double)__int_as_float(raw);
    return (raw & 0x7F800000) != 0x7F800000;
}

// int(v) of a finite double: truncation towards zero, saturated (as coord_of in posepaf_draw.hip)
__device__ __forceinline__ int trunc_i32(double v) {
    if (v >= 2147483648.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int)v;
}

struct alignas(4) Px4 {
    unsigned int v[3];   // four BGR pixels
};

// one listed instance, as the pixels need it
struct Inst {
    double a, c, s;      // semi-axis, cos, sin
    int cx, cy;          // ellipse centre
    int r0x, r0y, r1x, r1y;   // ring centres
    unsigned box;        // the instance's box clipped to the tile: x0 | x1 << 6 | y0 << 12 | y1 << 16 | type << 20
};

__device__ __forceinline__ bool ring_hit(int x, int y, int rx, int ry) {
    const long ddx = (long)x - rx, ddy = (long)y - ry;
    if (ddx < -5 || ddx > 5 || ddy < -5 || ddy > 5) return false;
    const long d2 = ddx * ddx + ddy * ddy;
    return d2 >= 9 && d2 <= 25;
}

__device__ __forceinline__ bool ellipse_hit(int x, int y, const Inst &in) {
    const double fx = (double)x - (double)in.cx, fy = (double)y - (double)in.cy;
    const double u0 = fx * in.c, u1 = fy * in.s, v0 = (-fx) * in.s, v1 = fy * in.c;
    const double u = u0 + u1, v = v0 + v1;
    const double p = u / in.a, q = v / 3.0;
    const double pp = p * p, qq = q * q;
    return pp + qq <= 1.0;
}

__device__ __forceinline__ unsigned blend(unsigned px, unsigned cur) {
    const double t0 = (double)px * 0.4, t1 = (double)cur * 0.6;
    return (unsigned)fmin(fmax(rint(t0 + t1), 0.0), 255.0);
}

template <bool VEC>
__global__ __launch_bounds__(LB_THREADS) void k_draw_limbs(const pp_record *__restrict__ recs, const unsigned char *src,
                                                           unsigned char *dst, const int *__restrict__ sizes, int batch, int hp,
                                                           int wp, int tiles_x, const double *__restrict__ tab) {
    __shared__ Inst s_inst[LB_THREADS];
    __shared__ int s_count[LB_THREADS / 64];

    const int tid = threadIdx.x;
    const int tile_x0 = (int)(blockIdx.x % tiles_x) * LB_TW, tile_y0 = (int)(blockIdx.x / tiles_x) * LB_TH;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        int h = hp, w = wp;
        if (sizes) {
            h = min(max(sizes[b], 0), hp);
            w = min(max(sizes[batch + b], 0), wp);
        }
        if (tile_x0 >= w || tile_y0 >= h) continue;               // uniform: nothing of this image in the tile
        const int tile_x1 = min(tile_x0 + LB_TW, w) - 1, tile_y1 = min(tile_y0 + LB_TH, h) - 1;   // inclusive
        const pp_record *rec = recs + b;
        const int nh = min(max(rec->n_humans, 0), PP_MAX_HUMANS);
        const bool is_float = (rec->status & PP_ST_FLOAT_COORDS) != 0;

        // ---- the thread's four pixels, one byte per channel
        const int lx = (tid & 15) * 4, ly = tid >> 4;
        const int x = tile_x0 + lx, y = tile_y0 + ly;
        const int npx = (y < h) ? min(max(w - x, 0), 4) : 0;      // pixels of this thread inside the image
        const long off = (((long)b * hp + y) * wp + x) * 3;
        Px4 px;
        px.v[0] = px.v[1] = px.v[2] = 0;
        const bool vec = VEC && npx == 4;
        if (vec) {
            px = *reinterpret_cast<const Px4 *>(src + off);
        } else {
            for (int i = 0; i < npx * 3; i++) {
                const int sh = (i & 3) * 8;
                px.v[i >> 2] |= (unsigned)src[off + i] << sh;
            }
        }
        unsigned ch[4][3];
#pragma unroll
        for (int i = 0; i < 12; i++) ch[i / 3][i % 3] = (px.v[i >> 2] >> ((i & 3) * 8)) & 0xFFu;
        bool changed = false;

        // ---- instances e = t * nh + human in draw order, LB_THREADS at a time
        const int total = LB_TYPES * nh;
        for (int base = 0; base < total; base += LB_THREADS) {
            const int e = base + tid;
            bool keep = false;
            Inst in;
            if (e < total) {
                const int t = e / nh, hid = e - t * nh;
                const pp_human *hm = rec->humans + hid;
                const int pa = d_limb_pairs[t][0], pb = d_limb_pairs[t][1];
                double X0, Y0, X1, Y1;
                if (hm->peak_id[pa] >= 0 && hm->peak_id[pb] >= 0 && coord_f64(hm->x[pa], is_float, X0) &&
                    coord_f64(hm->y[pa], is_float, Y0) && coord_f64(hm->x[pb], is_float, X1) && coord_f64(hm->y[pb], is_float, Y1)) {
                    const double dy = Y0 - Y1, dx = X0 - X1;
                    const double d0 = dy * dy, d1 = dx * dx;
                    const double half = sqrt(d0 + d1) / 2.0;
                    in.a = fmax(half >= 2147483647.0 ? 2147483647.0 : (double)(int)half, 0.5);
                    in.cx = trunc_i32((X0 + X1) / 2.0), in.cy = trunc_i32((Y0 + Y1) / 2.0);
                    in.r0x = trunc_i32(X0), in.r0y = trunc_i32(Y0), in.r1x = trunc_i32(X1), in.r1y = trunc_i32(Y1);
                    const long er = (long)fmax(in.a, 3.0) + 1;    // the ellipse lies within max(a, b) of its centre
                    const long bx0 = min(min((long)in.r0x, (long)in.r1x) - 6, (long)in.cx - er);
                    const long bx1 = max(max((long)in.r0x, (long)in.r1x) + 6, (long)in.cx + er);
                    const long by0 = min(min((long)in.r0y, (long)in.r1y) - 6, (long)in.cy - er);
                    const long by1 = max(max((long)in.r0y, (long)in.r1y) + 6, (long)in.cy + er);
                    if (bx1 >= tile_x0 && bx0 <= tile_x1 && by1 >= tile_y0 && by0 <= tile_y1) {
                        keep = true;
                        const unsigned cx0 = (unsigned)(max(bx0, (long)tile_x0) - tile_x0), cx1 = (unsigned)(min(bx1, (long)tile_x1) - tile_x0);
                        const unsigned cy0 = (unsigned)(max(by0, (long)tile_y0) - tile_y0), cy1 = (unsigned)(min(by1, (long)tile_y1) - tile_y0);
                        in.box = cx0 | (cx1 << 6) | (cy0 << 12) | (cy1 << 16) | ((unsigned)t << 20);
                        const int k = limb_angle_deg(dy, dx, tab);
                        in.c = tab[2 * (k + 180)], in.s = tab[2 * (k + 180) + 1];
                    }
                }
            }
            // kept instances, compacted in order: waves in thread order, lanes in lane order
            const unsigned long long m = __ballot(keep);
            if ((tid & 63) == 0) s_count[tid >> 6] = __popcll(m);
            __syncthreads();
            int before = 0, cnt = 0;
#pragma unroll
            for (int wv = 0; wv < LB_THREADS / 64; wv++) {
                const int c = s_count[wv];
                if (wv < (tid >> 6)) before += c;
                cnt += c;
            }
            if (keep) s_inst[before + __popcll(m & ((1ull << (tid & 63)) - 1ull))] = in;
            __syncthreads();

            // ---- the fold, forwards
            if (npx > 0) {
                for (int i = 0; i < cnt; i++) {
                    const unsigned box = s_inst[i].box;
                    const int cx0 = box & 63, cx1 = (box >> 6) & 63, cy0 = (box >> 12) & 15, cy1 = (box >> 16) & 15;
                    if (ly < cy0 || ly > cy1 || lx + 3 < cx0 || lx > cx1) continue;
                    const Inst ins = s_inst[i];
                    const unsigned char *colour = d_limb_colors[(box >> 20) & 31];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (k >= npx || lx + k < cx0 || lx + k > cx1) continue;
                        const bool el = ellipse_hit(x + k, y, ins);
                        if (!(el || ring_hit(x + k, y, ins.r0x, ins.r0y) || ring_hit(x + k, y, ins.r1x, ins.r1y))) continue;
#pragma unroll
                        for (int j = 0; j < 3; j++) ch[k][j] = blend(ch[k][j], el ? (unsigned)colour[j] : 0u);
                        changed = true;
                    }
                }
            }
            __syncthreads();                                       // the list is rewritten by the next chunk
        }

        // ---- store: the image's own pixels only; in place, untouched pixels are not written again
        if (npx > 0 && (dst != src || changed)) {
            px.v[0] = px.v[1] = px.v[2] = 0;
#pragma unroll
            for (int i = 0; i < 12; i++) px.v[i >> 2] |= ch[i / 3][i % 3] << ((i & 3) * 8);
            if (vec) {
                *reinterpret_cast<Px4 *>(dst + off) = px;
            } else {
                for (int i = 0; i < npx * 3; i++) dst[off + i] = (unsigned char)(px.v[i >> 2] >> ((i & 3) * 8));
            }
        }
    }
}
}  // namespace

extern "C" int pp_limb_angle_table(double *table_host) {
    if (!table_host) return PP_ERR_BAD_ARG;
    fill_angle_table(table_host);
    return PP_OK;
}

extern "C" int pp_limb_angle_deg(double dy, double dx) { return limb_angle_deg(dy, dx, host_angle_table()); }

extern "C" int pp_draw_limbs_u8(const pp_record *records_dev, const void *src_u8, void *dst_u8, const int *sizes_dev, int batch,
                                int hp, int wp, const double *angle_table_dev, void *stream) {
    if (!records_dev || !src_u8 || !dst_u8 || !angle_table_dev || batch <= 0 || hp <= 0 || wp <= 0) return PP_ERR_BAD_ARG;
    const long tiles_x = ((long)wp + LB_TW - 1) / LB_TW, tiles_y = ((long)hp + LB_TH - 1) / LB_TH;
    if (tiles_x * tiles_y > 2147483647L) return PP_ERR_BAD_ARG;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(batch < 65535 ? batch : 65535)), block(LB_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char *src = static_cast<const unsigned char *>(src_u8);
    unsigned char *dst = static_cast<unsigned char *>(dst_u8);
    // 12-byte accesses need every 4-pixel group 4-byte aligned: both bases and the row pitch (true of every engine bucket)
    const bool vec = ((long)wp * 3) % 4 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(k_draw_limbs<true>, grid, block, 0, st, records_dev, src, dst, sizes_dev, batch, hp, wp, (int)tiles_x,
                           angle_table_dev);
    else
        hipLaunchKernelGGL(k_draw_limbs<false>, grid, block, 0, st, records_dev, src, dst, sizes_dev, batch, hp, wp, (int)tiles_x,
                           angle_table_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
