// posepaf_draw.hip -- the record-based skeleton drawing of the demo (reference demo_image.py:174-192, utils/common.py:240-264
// with pixel coordinates) for a whole bucket in one launch, straight from pp_record[b] in device memory, BIT-EQUAL to the NumPy
// renderer utils/draw.py:draw_humans(canvas, humans, normalized=False):
//   per human, in order: the present joints 0..17 as discs   (x - cx)^2 + (y - cy)^2 <= 20.25          colour CocoColors[part]
//                        then CocoPairsRender 0..16 as lines  d2 <= 2.25 with, in float64, one operation at a time,
//                            u  = clip(((x - ax) * dx + (y - ay) * dy) / den, 0, 1)     (u = 0 when den == 0)
//                            d2 = (x - (ax + u * dx))^2 + (y - (ay + u * dy))^2                         colour CocoColors[pair]
// Painting is "later overwrites earlier", so a pixel ends with the colour of the LAST primitive in draw order whose test holds
// and is unchanged when none holds; draw.py's bounding boxes never cut a primitive (tests/test_draw_records_cpu.py).  That makes
// every pixel independent: a workgroup takes one 64 x 16 tile of one image, keeps the humans whose joints (+- 5 px) reach the
// tile, lists their primitives chunk by chunk in LDS, and every thread walks the list BACKWARDS for its four pixels until each
// has met its first hit.  No atomics, no memset, no allocation, nothing shared between workgroups.
// Compiled with -ffp-contract=off (csrc/Makefile STRICT): products and sums round separately, the f64 division is hipcc's
// correctly rounded one -- the same IEEE operations NumPy evaluates.  Exact for coordinates within +-32767; beyond that the
// clipping below is done in 64 bits and nothing outside the image's own pixels is ever written.
#include <hip/hip_runtime.h>

#include "../../include/posepaf.h"

namespace {

constexpr int DR_TW = 64, DR_TH = 16;        // tile: 16 threads x 4 pixels wide, 16 rows
constexpr int DR_THREADS = 256;
constexpr int DR_PRIMS = 35;                 // 18 discs + 17 lines per human
constexpr int DR_CHUNK = DR_THREADS / DR_PRIMS;   // 7 humans' primitives per pass over the LDS list
constexpr unsigned DR_NONE = 0xFFFFFFFFu;

// utils/common.py:281-283 (B, G, R)
__device__ const unsigned char d_colors[PP_NUM_PART][3] = {
    {255, 0, 0},   {255, 85, 0},  {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0},  {0, 255, 0},   {0, 255, 85},  {0, 255, 170},
    {0, 255, 255}, {0, 170, 255}, {0, 85, 255},  {0, 0, 255},   {85, 0, 255},  {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}};
// utils/common.py:285-289 CocoPairsRender = CocoPairs[:-2]
__device__ const signed char d_pairs[17][2] = {{1, 2}, {1, 5},   {2, 3},   {3, 4},   {5, 6}, {6, 7},  {1, 8},   {8, 9},  {9, 10},
                                               {1, 11}, {11, 12}, {12, 13}, {1, 0}, {0, 14}, {14, 16}, {0, 15}, {15, 17}};

// int(bp.x) of a float32 coordinate: truncation towards zero (saturated; NaN -> 0: Python would raise there)
__device__ __forceinline__ int coord_of(int raw, bool is_float) {
    if (!is_float) return raw;
    const float f = __int_as_float(raw);
    if (!(f == f)) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int)f;
}

__device__ __forceinline__ bool line_hit(int x, int y, int ax, int ay, int bx, int by) {
    const double dx = (double)bx - (double)ax, dy = (double)by - (double)ay;
    const double den = dx * dx + dy * dy;
    const double px = (double)x - (double)ax, py = (double)y - (double)ay;
    double u = 0.0;
    if (den > 0.0) {
        const double t0 = px * dx, t1 = py * dy;
        u = (t0 + t1) / den;
        u = fmin(fmax(u, 0.0), 1.0);
    }
    const double ex = (double)x - ((double)ax + u * dx), ey = (double)y - ((double)ay + u * dy);
    const double e0 = ex * ex, e1 = ey * ey;
    return e0 + e1 <= 2.25;
}

struct alignas(4) Px4 {
    unsigned int v[3];   // four BGR pixels
};

__device__ __forceinline__ void put_px(Px4 &p, int k, const unsigned char *c) {
    // pixel k occupies bytes 3k .. 3k + 2 of the 12
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int byte = 3 * k + j;
        const int sh = (byte & 3) * 8;
        p.v[byte >> 2] = (p.v[byte >> 2] & ~(0xFFu << sh)) | ((unsigned)c[j] << sh);
    }
}

template <bool VEC>
__global__ __launch_bounds__(DR_THREADS) void k_draw_humans(const pp_record *__restrict__ recs, const unsigned char *src,
                                                            unsigned char *dst, const int *__restrict__ sizes, int batch, int hp,
                                                            int wp, int tiles_x) {
    __shared__ unsigned long long s_mask[2];
    __shared__ unsigned char s_list[PP_MAX_HUMANS];
    __shared__ int s_ax[DR_THREADS], s_ay[DR_THREADS], s_bx[DR_THREADS], s_by[DR_THREADS];
    __shared__ unsigned s_meta[DR_THREADS];

    const int tid = threadIdx.x;
    const int tile_x0 = (int)(blockIdx.x % tiles_x) * DR_TW, tile_y0 = (int)(blockIdx.x / tiles_x) * DR_TH;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        int h = hp, w = wp;
        if (sizes) {
            h = min(max(sizes[b], 0), hp);
            w = min(max(sizes[batch + b], 0), wp);
        }
        if (tile_x0 >= w || tile_y0 >= h) continue;               // uniform: nothing of this image in the tile
        const int tile_x1 = min(tile_x0 + DR_TW, w) - 1, tile_y1 = min(tile_y0 + DR_TH, h) - 1;   // inclusive
        const pp_record *rec = recs + b;
        const int nh = min(max(rec->n_humans, 0), PP_MAX_HUMANS);
        const bool is_float = (rec->status & PP_ST_FLOAT_COORDS) != 0;

        // ---- the thread's four pixels
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

        // ---- humans whose present joints, grown by 5 px, reach the tile: ordered list in LDS
        bool keep = false;
        if (tid < nh) {
            const pp_human *hm = rec->humans + tid;
            int x0 = 2147483647, y0 = 2147483647, x1 = -2147483647 - 1, y1 = -2147483647 - 1;
            bool any = false;
            for (int p = 0; p < PP_NUM_PART; p++) {
                if (hm->peak_id[p] < 0) continue;
                const int cx = coord_of(hm->x[p], is_float), cy = coord_of(hm->y[p], is_float);
                x0 = min(x0, cx), x1 = max(x1, cx), y0 = min(y0, cy), y1 = max(y1, cy);
                any = true;
            }
            keep = any && (long)x1 + 5 >= tile_x0 && (long)x0 - 5 <= tile_x1 && (long)y1 + 5 >= tile_y0 && (long)y0 - 5 <= tile_y1;
        }
        const unsigned long long m = __ballot(keep);
        if (tid < 128 && (tid & 63) == 0) s_mask[tid >> 6] = m;
        __syncthreads();
        const int n0 = __popcll(s_mask[0]);
        const int nsurv = n0 + __popcll(s_mask[1]);
        if (keep) {
            const unsigned long long below = m & ((1ull << (tid & 63)) - 1ull);
            s_list[(tid >= 64 ? n0 : 0) + __popcll(below)] = (unsigned char)tid;
        }
        __syncthreads();

        // ---- the survivors' primitives, 7 humans at a time from the LAST one back; each pixel stops at its first hit
        unsigned done = npx >= 4 ? 0u : (0xFu << npx) & 0xFu;      // bit k: pixel k needs no more tests
        unsigned col = 0;                                           // byte k: colour index of pixel k's hit
        unsigned hitmask = 0;
        for (int top = nsurv; top > 0; top -= DR_CHUNK) {
            const int lo = max(top - DR_CHUNK, 0), cnt = top - lo;
            if (tid < cnt * DR_PRIMS) {
                const int j = tid / DR_PRIMS, p = tid - j * DR_PRIMS;
                const pp_human *hm = rec->humans + s_list[lo + j];
                unsigned meta = DR_NONE;
                int ax = 0, ay = 0, bx = 0, by = 0;
                long bx0, bx1, by0, by1;
                bool present;
                if (p < PP_NUM_PART) {
                    present = hm->peak_id[p] >= 0;
                    if (present) {
                        ax = bx = coord_of(hm->x[p], is_float);
                        ay = by = coord_of(hm->y[p], is_float);
                    }
                    bx0 = (long)ax - 4, bx1 = (long)ax + 4, by0 = (long)ay - 4, by1 = (long)ay + 4;   // 4^2 + 2^2 = 20 <= 20.25 < 5^2
                } else {
                    const int a = d_pairs[p - PP_NUM_PART][0], c = d_pairs[p - PP_NUM_PART][1];
                    present = hm->peak_id[a] >= 0 && hm->peak_id[c] >= 0;
                    if (present) {
                        ax = coord_of(hm->x[a], is_float), ay = coord_of(hm->y[a], is_float);
                        bx = coord_of(hm->x[c], is_float), by = coord_of(hm->y[c], is_float);
                    }
                    bx0 = (long)min(ax, bx) - 2, bx1 = (long)max(ax, bx) + 2;                        // d2 <= 2.25: within 1.5 px
                    by0 = (long)min(ay, by) - 2, by1 = (long)max(ay, by) + 2;
                }
                if (present && bx1 >= tile_x0 && bx0 <= tile_x1 && by1 >= tile_y0 && by0 <= tile_y1) {
                    const unsigned cx0 = (unsigned)(max(bx0, (long)tile_x0) - tile_x0), cx1 = (unsigned)(min(bx1, (long)tile_x1) - tile_x0);
                    const unsigned cy0 = (unsigned)(max(by0, (long)tile_y0) - tile_y0), cy1 = (unsigned)(min(by1, (long)tile_y1) - tile_y0);
                    const unsigned kind = p < PP_NUM_PART ? 0u : 1u, ci = p < PP_NUM_PART ? (unsigned)p : (unsigned)(p - PP_NUM_PART);
                    meta = cx0 | (cx1 << 6) | (cy0 << 12) | (cy1 << 16) | (ci << 20) | (kind << 25);
                }
                s_ax[tid] = ax, s_ay[tid] = ay, s_bx[tid] = bx, s_by[tid] = by;
                s_meta[tid] = meta;
            }
            __syncthreads();
            if (done != 0xFu) {
                for (int e = cnt * DR_PRIMS - 1; e >= 0; e--) {
                    const unsigned meta = s_meta[e];
                    if (meta == DR_NONE) continue;
                    const int cx0 = meta & 63, cx1 = (meta >> 6) & 63, cy0 = (meta >> 12) & 15, cy1 = (meta >> 16) & 15;
                    if (ly < cy0 || ly > cy1 || lx + 3 < cx0 || lx > cx1) continue;
                    const int ax = s_ax[e], ay = s_ay[e];
                    const unsigned ci = (meta >> 20) & 31;
                    if ((meta >> 25) & 1) {
                        const int bx = s_bx[e], by = s_by[e];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if ((done >> k) & 1 || lx + k < cx0 || lx + k > cx1) continue;
                            if (line_hit(x + k, y, ax, ay, bx, by)) done |= 1u << k, hitmask |= 1u << k, col |= ci << (8 * k);
                        }
                    } else {
                        const int ddy = y - ay;       // the clipped box puts the centre within 4 px of the pixel: no overflow
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            if ((done >> k) & 1 || lx + k < cx0 || lx + k > cx1) continue;
                            const int ddx = x + k - ax;
                            if (ddx * ddx + ddy * ddy <= 20) done |= 1u << k, hitmask |= 1u << k, col |= ci << (8 * k);
                        }
                    }
                    if (done == 0xFu) break;
                }
            }
            __syncthreads();
        }

        // ---- paint and store: the image's own pixels only; in place, untouched pixels are not written again
#pragma unroll
        for (int k = 0; k < 4; k++)
            if ((hitmask >> k) & 1) put_px(px, k, d_colors[(col >> (8 * k)) & 31]);
        if (npx > 0 && (dst != src || hitmask)) {
            if (vec) {
                *reinterpret_cast<Px4 *>(dst + off) = px;
            } else {
                for (int i = 0; i < npx * 3; i++) dst[off + i] = (unsigned char)(px.v[i >> 2] >> ((i & 3) * 8));
            }
        }
    }
}
}  // namespace

extern "C" int pp_draw_humans_u8(const pp_record *records_dev, const void *src_u8, void *dst_u8, const int *sizes_dev, int batch,
                                 int hp, int wp, void *stream) {
    if (!records_dev || !src_u8 || !dst_u8 || batch <= 0 || hp <= 0 || wp <= 0) return PP_ERR_BAD_ARG;
    const long tiles_x = ((long)wp + DR_TW - 1) / DR_TW, tiles_y = ((long)hp + DR_TH - 1) / DR_TH;
    if (tiles_x * tiles_y > 2147483647L) return PP_ERR_BAD_ARG;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)(batch < 65535 ? batch : 65535)), block(DR_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned char *src = static_cast<const unsigned char *>(src_u8);
    unsigned char *dst = static_cast<unsigned char *>(dst_u8);
    // 12-byte accesses need every 4-pixel group 4-byte aligned: both bases and the row pitch (true of every engine bucket)
    const bool vec = ((long)wp * 3) % 4 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0;
    if (vec)
        hipLaunchKernelGGL(k_draw_humans<true>, grid, block, 0, st, records_dev, src, dst, sizes_dev, batch, hp, wp, (int)tiles_x);
    else
        hipLaunchKernelGGL(k_draw_humans<false>, grid, block, 0, st, records_dev, src, dst, sizes_dev, batch, hp, wp, (int)tiles_x);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
