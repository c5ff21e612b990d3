// posepaf_loss.hip -- the reference's multi-scale focal-L2 validation loss (models/loss_model.py:23-81, :133-161) as per-image terms:
//   terms[t][s][b] = sum over c, y, x of  (p - G)^2 * |1 - st| * M * cw[c]          (PP_LOSS_PLAIN_L2: without |1 - st|, :103-131)
//   G   adaptive_avg_pool2d of the target to the prediction's (h_s, w_s): window rows floor(i H / h_s) .. ceil((i + 1) H / h_s),
//       columns alike; summed in float64 in row-major order, divided by the cell count in float64, rounded ONCE to float32
//   st  p where G >= 0.01f (a float32 comparison, as torch compares a float32 tensor with the scalar), 1 - p elsewhere
//   M   the mask resampled bilinearly with align_corners = False (source coordinate max((i + 0.5) H / h_s - 0.5, 0), second tap
//       clamped to the last row / column), in float64 from the float32 mask values; values < 0.5 become 0; all ones without a mask
//   cw  multi_task_weight for channel 48, keypoint_task_weight for channels 30..47, 1 otherwise
// Everything behind G and M is float64; p is widened from its stored binary16 / float32 value.  Compiled with -ffp-contract=off.
// A workgroup takes LS_P consecutive pixels (row-major) of one prediction scale of one image: in the pixel-major layouts that is one
// contiguous run of memory, in the planar layout one run per channel.  It pools the target for all 50 channels and resamples the
// mask ONCE into LDS, then walks the stacks, so one G serves every stack.  A thread owns groups of 8 consecutive stored elements
// (one 16-byte load for binary16, two for float32; element by element where the run is not 16-byte aligned or at its end -- the SAME
// elements in the same order either way), adds its terms in element order into one float64 accumulator per stack, the wave adds by
// a fixed butterfly, the four wave sums are added in wave order, and the workgroup's partial goes to the workspace with a plain
// store.  k_focal_l2_finish adds an image's partials of one (stack, scale) in tile order.  No atomics, no memset: the order depends
// on the shapes alone, so an image's terms are bit-identical in every batch, slot and run.
//
// k_focal_l2_grad is the derivative with respect to the predictions, with the same tiling and the same G and M (stage_target /
// stage_mask).  Given tw = dL/dterms[t][s][b] (float64) it stores, for every element,
//   d = p - (double)G;   focal: f = |1 - st|,  f' = -sgn(1 - p) where G >= 0.01f, sgn(p) elsewhere (sgn(0) = +0.0: torch's abs
//   backward), e = (2.0 d) f + (d d) f';   plain: e = 2.0 d;   grad = tw (cw (M e)), in exactly this association,
// rounded to float32 (nearest even) and, for binary16 predictions, that float32 to binary16.  The gradients have the predictions'
// geometry; a thread stores the groups it would load, 16 bytes at a time under the same rule and element by element elsewhere,
// channels 0..49 only.  Elementwise: no reduction, no workspace, nothing depends on batch, slot or launch geometry.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "posepaf_internal.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_P = 128;                   // pixels of a tile
constexpr int LS_PS = LS_P + 1;             // LDS row of one channel (padded: the pixel-major walk strides over channels)
constexpr int LS_V = 8;                     // stored elements of one group
constexpr int LS_CH = 50;
constexpr int LS_MAX_STACKS = 8, LS_MAX_SCALES = 5;
constexpr long long LS_MAX_PIXELS = 1ll << 30;

struct LossTiles {
    int first[LS_MAX_SCALES + 1];           // first tile of every scale; first[n_scales] = tiles of one image
};

struct LossArgs {                           // travels by value in the kernel arguments
    const void *pred[LS_MAX_STACKS * LS_MAX_SCALES];   // [t * n_scales + s]
    int hs[LS_MAX_SCALES], ws[LS_MAX_SCALES];
    LossTiles tiles;
    unsigned vec;                           // bit s: every stack's scale-s tensor may be read with 16-byte loads
};

struct GradPtrs {                           // travels by value in the kernel arguments
    void *grad[LS_MAX_STACKS * LS_MAX_SCALES];         // [t * n_scales + s], the geometry of pred[t * n_scales + s]
};

__device__ __forceinline__ double widen(float v) { return (double)v; }
__device__ __forceinline__ double widen(__half v) { return (double)__half2float(v); }

struct alignas(16) Quad {
    unsigned v[4];
};

// the n <= 8 stored elements p[0 .. n) widened to float64 (entries past n: 0, never used)
__device__ __forceinline__ void load_group(const __half *p, int n, bool vec, double out[LS_V]) {
    if (vec && n == LS_V) {
        const Quad q = *reinterpret_cast<const Quad *>(p);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const __half2 h2 = *reinterpret_cast<const __half2 *>(&q.v[j]);
            out[2 * j] = (double)__low2float(h2), out[2 * j + 1] = (double)__high2float(h2);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < LS_V; j++) out[j] = j < n ? widen(p[j]) : 0.0;
}

__device__ __forceinline__ void load_group(const float *p, int n, bool vec, double out[LS_V]) {
    if (vec && n == LS_V) {
        const Quad q0 = *reinterpret_cast<const Quad *>(p), q1 = *reinterpret_cast<const Quad *>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; j++) out[j] = (double)__uint_as_float(q0.v[j]), out[4 + j] = (double)__uint_as_float(q1.v[j]);
        return;
    }
#pragma unroll
    for (int j = 0; j < LS_V; j++) out[j] = j < n ? widen(p[j]) : 0.0;
}

__device__ __forceinline__ double channel_weight(int c, double mtw, double kpw) {
    return c == LS_CH - 2 ? mtw : (c >= PP_NUM_LIMB && c < PP_NUM_LIMB + PP_NUM_PART ? kpw : 1.0);
}

__device__ __forceinline__ double loss_term(double p, float g, double m, double cw, bool plain) {
    const double d = p - (double)g;
    double v = d * d;
    if (!plain) {
        const double st = g >= 0.01f ? p : 1.0 - p;
        v = v * fabs(1.0 - st);
    }
    return v * m * cw;
}

// the pooled target of a tile, all channels, into s_g[c * LS_PS + i]: thread -> pixel tid % LS_P (consecutive lanes, consecutive
// pixels), channels tid / LS_P, + 2, + 4 ...  (both kernels stage through these two functions: one definition of G and M)
template <typename TT>
__device__ __forceinline__ void stage_target(float *s_g, const TT *target, long long target_image_stride, int b, int H, int W, int h,
                                             int w, int p0, int npx, int tid) {
    const int i = tid & (LS_P - 1);
    int r0 = 0, r1 = 0, c0 = 0, c1 = 0;
    if (i < npx) {
        const int p = p0 + i, y = p / w, x = p - y * w;
        r0 = (int)(((long long)y * H) / h), r1 = (int)((((long long)y + 1) * H + h - 1) / h);
        c0 = (int)(((long long)x * W) / w), c1 = (int)((((long long)x + 1) * W + w - 1) / w);
    }
    const double cells = (double)((long long)(r1 - r0) * (c1 - c0));
    const TT *tb = target + (size_t)b * (size_t)target_image_stride;
    for (int c = tid / LS_P; c < LS_CH; c += LS_THREADS / LS_P) {
        float g = 0.0f;
        if (i < npx) {
            const TT *plane = tb + (size_t)c * H * W;
            double sum = 0.0;
            for (int r = r0; r < r1; r++) {
                const TT *row = plane + (size_t)r * W;
                for (int q = c0; q < c1; q++) sum += widen(row[q]);
            }
            g = (float)(sum / cells);
        }
        s_g[c * LS_PS + i] = g;
    }
}

// the resampled, thresholded mask of a tile into s_m[i] (0 behind the tile's last pixel)
__device__ __forceinline__ void stage_mask(double *s_m, const float *mask, int b, int H, int W, int h, int w, int p0, int npx,
                                           int tid) {
    if (tid < LS_P) {
        double m = 0.0;
        if (tid < npx) {
            m = 1.0;
            if (mask) {
                const int p = p0 + tid, y = p / w, x = p - y * w;
                const double sy = fmax(((double)y + 0.5) * (double)H / (double)h - 0.5, 0.0);
                const double sx = fmax(((double)x + 0.5) * (double)W / (double)w - 0.5, 0.0);
                const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
                const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
                const double ly1 = sy - (double)y0, lx1 = sx - (double)x0;
                const double ly0 = 1.0 - ly1, lx0 = 1.0 - lx1;
                const float *mb = mask + (size_t)b * H * W;
                const double m00 = (double)mb[(size_t)y0 * W + x0], m01 = (double)mb[(size_t)y0 * W + x1];
                const double m10 = (double)mb[(size_t)y1 * W + x0], m11 = (double)mb[(size_t)y1 * W + x1];
                m = ly0 * (lx0 * m00 + lx1 * m01) + ly1 * (lx0 * m10 + lx1 * m11);
                if (m < 0.5) m = 0.0;
            }
        }
        s_m[tid] = m;
    }
}

// MODE 0: planes (batch, 50, h, w); 1: pixel-major with 64 elements per pixel; 2: pixel-major with `stride` >= 50 elements per pixel
template <typename TP, typename TT, int MODE>
__global__ __launch_bounds__(LS_THREADS) void k_focal_l2(LossArgs a, int stride, const TT *__restrict__ target, long long target_image_stride,
                                                          const float *__restrict__ mask, int batch, int H, int W, int n_stacks,
                                                          int n_scales, double mtw, double kpw, int flags, double *__restrict__ partial) {
    __shared__ float s_g[LS_CH * LS_PS];
    __shared__ double s_m[LS_P];
    __shared__ double s_red[LS_THREADS / 64];

    const int tid = threadIdx.x;
    // image fastest, tiles in DESCENDING order: the coarse scales' workgroups, whose threads walk whole pooling windows alone, start
    // first and run under the many short fine-scale ones instead of forming the tail
    const int b = (int)(blockIdx.x % (unsigned)batch), tile = a.tiles.first[n_scales] - 1 - (int)(blockIdx.x / (unsigned)batch);
    int s = 0;
    while (s + 1 < n_scales && tile >= a.tiles.first[s + 1]) s++;
    const int h = a.hs[s], w = a.ws[s];
    const int p0 = (tile - a.tiles.first[s]) * LS_P;
    const int npx = min(LS_P, h * w - p0);                    // >= 1: the host launches ceil(h w / LS_P) tiles per scale

    stage_target(s_g, target, target_image_stride, b, H, W, h, w, p0, npx, tid);
    stage_mask(s_m, mask, b, H, W, h, w, p0, npx, tid);
    __syncthreads();

    const bool plain = (flags & PP_LOSS_PLAIN_L2) != 0;
    const bool vec = ((a.vec >> s) & 1u) != 0;
    const size_t hw = (size_t)h * w;
    const int tiles_per_image = a.tiles.first[n_scales];
    for (int t = 0; t < n_stacks; t++) {
        const TP *pb = static_cast<const TP *>(a.pred[t * n_scales + s]);
        double acc = 0.0;
        double v[LS_V];
        if (MODE == 0) {
            const int gpc = (npx + LS_V - 1) / LS_V;                 // groups per channel
            const TP *base = pb + (size_t)b * LS_CH * hw + p0;
            for (int g = tid; g < LS_CH * gpc; g += LS_THREADS) {
                const int c = g / gpc, i0 = (g - c * gpc) * LS_V;
                const int n = min(LS_V, npx - i0);
                load_group(base + (size_t)c * hw + i0, n, vec, v);
                const double cw = channel_weight(c, mtw, kpw);
#pragma unroll
                for (int j = 0; j < LS_V; j++)
                    if (j < n) acc += loss_term(v[j], s_g[c * LS_PS + i0 + j], s_m[i0 + j], cw, plain);
            }
        } else {
            // the tile's run of memory, up to channel 49 of its last pixel (nothing behind it is ever addressed)
            const int len = (npx - 1) * stride + LS_CH;
            const TP *base = pb + ((size_t)b * hw + p0) * (size_t)stride;
            const int ng = (len + LS_V - 1) / LS_V;
            for (int g = tid; g < ng; g += LS_THREADS) {
                const int e0 = g * LS_V;
                int i, c;
                if (MODE == 1) {
                    i = e0 >> 6, c = e0 & 63;
                    if (c >= LS_CH) continue;                         // a whole group of padding channels
                } else {
                    i = e0 / stride, c = e0 - i * stride;
                }
                const int n = min(LS_V, len - e0);
                load_group(base + e0, n, vec, v);
#pragma unroll
                for (int j = 0; j < LS_V; j++) {
                    if (j < n && c < LS_CH) acc += loss_term(v[j], s_g[c * LS_PS + i], s_m[i], channel_weight(c, mtw, kpw), plain);
                    if (++c == stride) c = 0, i++;
                }
            }
        }
        // ---- fixed-order reduction: butterfly inside the wave, the four waves in order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if ((tid & 63) == 0) s_red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0)
            partial[((size_t)b * tiles_per_image + tile) * n_stacks + t] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
        __syncthreads();
    }
}

// terms[t][s][b] = the partials of image b's scale-s tiles for stack t, added in tile order
__global__ __launch_bounds__(LS_THREADS) void k_focal_l2_finish(LossTiles tiles, const double *__restrict__ partial, int batch, int n_stacks,
                                                                 int n_scales, double *__restrict__ terms) {
    const long long idx = (long long)blockIdx.x * LS_THREADS + threadIdx.x;
    if (idx >= (long long)n_stacks * n_scales * batch) return;
    const int b = (int)(idx % batch), s = (int)((idx / batch) % n_scales), t = (int)(idx / ((long long)batch * n_scales));
    const int tiles_per_image = tiles.first[n_scales];
    double sum = 0.0;
    for (int tile = tiles.first[s]; tile < tiles.first[s + 1]; tile++) sum += partial[((size_t)b * tiles_per_image + tile) * n_stacks + t];
    terms[idx] = sum;
}

__device__ __forceinline__ double sgn(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// d terms / d p of one element, times its upstream weight, rounded once to float32
__device__ __forceinline__ float grad_term(double p, float g, double m, double cw, double tw, bool plain) {
    const double d = p - (double)g;
    double e = 2.0 * d;
    if (!plain) {
        const bool fg = g >= 0.01f;
        const double f = fabs(1.0 - (fg ? p : 1.0 - p));
        const double fd = fg ? (1.0 - p > 0.0 ? -1.0 : (1.0 - p < 0.0 ? 1.0 : 0.0)) : sgn(p);
        e = e * f + (d * d) * fd;
    }
    return (float)(tw * (cw * (m * e)));
}

__device__ __forceinline__ void store_one(float *q, float v) { *q = v; }
__device__ __forceinline__ void store_one(__half *q, float v) { *q = __float2half_rn(v); }

// a whole group of LS_V elements with 16-byte stores (q 16-byte aligned)
__device__ __forceinline__ void store_group(__half *q, const float v[LS_V]) {
    Quad o;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const __half2 h2 = __halves2half2(__float2half_rn(v[2 * j]), __float2half_rn(v[2 * j + 1]));
        o.v[j] = *reinterpret_cast<const unsigned *>(&h2);
    }
    *reinterpret_cast<Quad *>(q) = o;
}

__device__ __forceinline__ void store_group(float *q, const float v[LS_V]) {
    Quad o0, o1;
#pragma unroll
    for (int j = 0; j < 4; j++) o0.v[j] = __float_as_uint(v[j]), o1.v[j] = __float_as_uint(v[4 + j]);
    *reinterpret_cast<Quad *>(q) = o0, *reinterpret_cast<Quad *>(q + 4) = o1;
}

// the gradient of sum_tsb tw[t][s][b] terms[t][s][b] with respect to every prediction element; grid, tiles and staging as k_focal_l2
template <typename TP, typename TT, int MODE>
__global__ __launch_bounds__(LS_THREADS) void k_focal_l2_grad(LossArgs a, GradPtrs gp, int stride, const TT *__restrict__ target,
                                                               long long target_image_stride, const float *__restrict__ mask, int batch, int H,
                                                               int W, int n_stacks, int n_scales, double mtw, double kpw, int flags,
                                                               const double *__restrict__ term_weight) {
    __shared__ float s_g[LS_CH * LS_PS];
    __shared__ double s_m[LS_P];

    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x % (unsigned)batch), tile = a.tiles.first[n_scales] - 1 - (int)(blockIdx.x / (unsigned)batch);
    int s = 0;
    while (s + 1 < n_scales && tile >= a.tiles.first[s + 1]) s++;
    const int h = a.hs[s], w = a.ws[s];
    const int p0 = (tile - a.tiles.first[s]) * LS_P;
    const int npx = min(LS_P, h * w - p0);

    stage_target(s_g, target, target_image_stride, b, H, W, h, w, p0, npx, tid);
    stage_mask(s_m, mask, b, H, W, h, w, p0, npx, tid);
    __syncthreads();

    const bool plain = (flags & PP_LOSS_PLAIN_L2) != 0;
    const bool vec = ((a.vec >> s) & 1u) != 0;               // the host clears the bit unless predictions AND gradients qualify
    const size_t hw = (size_t)h * w;
    for (int t = 0; t < n_stacks; t++) {
        const TP *pb = static_cast<const TP *>(a.pred[t * n_scales + s]);
        TP *gb = static_cast<TP *>(gp.grad[t * n_scales + s]);
        const double tw = term_weight[((size_t)t * n_scales + s) * batch + b];
        double v[LS_V];
        float o[LS_V];
        if (MODE == 0) {
            const int gpc = (npx + LS_V - 1) / LS_V;
            const size_t off = (size_t)b * LS_CH * hw + p0;
            for (int g = tid; g < LS_CH * gpc; g += LS_THREADS) {
                const int c = g / gpc, i0 = (g - c * gpc) * LS_V;
                const int n = min(LS_V, npx - i0);
                const size_t at = off + (size_t)c * hw + i0;
                load_group(pb + at, n, vec, v);
                const double cw = channel_weight(c, mtw, kpw);
#pragma unroll
                for (int j = 0; j < LS_V; j++)
                    o[j] = j < n ? grad_term(v[j], s_g[c * LS_PS + i0 + j], s_m[i0 + j], cw, tw, plain) : 0.0f;
                if (vec && n == LS_V) {
                    store_group(gb + at, o);
                } else {
#pragma unroll
                    for (int j = 0; j < LS_V; j++)
                        if (j < n) store_one(gb + at + j, o[j]);
                }
            }
        } else {
            const int len = (npx - 1) * stride + LS_CH;       // up to channel 49 of the tile's last pixel: nothing behind it is addressed
            const size_t off = ((size_t)b * hw + p0) * (size_t)stride;
            const int ng = (len + LS_V - 1) / LS_V;
            for (int g = tid; g < ng; g += LS_THREADS) {
                const int e0 = g * LS_V;
                int i, c;
                if (MODE == 1) {
                    i = e0 >> 6, c = e0 & 63;
                    if (c >= LS_CH) continue;                 // a whole group of padding channels: neither read nor written
                } else {
                    i = e0 / stride, c = e0 - i * stride;
                }
                const int n = min(LS_V, len - e0);
                load_group(pb + off + e0, n, vec, v);
                unsigned real = 0;                            // bit j: element j is one of channels 0..49 of a pixel of the tile
#pragma unroll
                for (int j = 0; j < LS_V; j++) {
                    o[j] = 0.0f;
                    if (j < n && c < LS_CH) {
                        o[j] = grad_term(v[j], s_g[c * LS_PS + i], s_m[i], channel_weight(c, mtw, kpw), tw, plain);
                        real |= 1u << j;
                    }
                    if (++c == stride) c = 0, i++;
                }
                if (vec && real == (1u << LS_V) - 1u) {
                    store_group(gb + off + e0, o);
                } else {                                      // a group that holds padding channels or ends the run: its real elements
#pragma unroll
                    for (int j = 0; j < LS_V; j++)
                        if ((real >> j) & 1u) store_one(gb + off + e0 + j, o[j]);
                }
            }
        }
    }
}

int device_present() {
    static int have = -1;
    if (have < 0) {
        int n = 0;
        have = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    }
    return have;
}

// the shape checks both entries share; fills the tile table.  PP_OK or the status to return
int plan_tiles(int batch, int n_stacks, int n_scales, const int *hs, const int *ws, LossTiles *tiles) {
    if (batch < 1 || n_stacks < 1 || n_scales < 1 || !hs || !ws) return PP_ERR_BAD_ARG;
    if (n_stacks > LS_MAX_STACKS || n_scales > LS_MAX_SCALES) return PP_ERR_UNSUPPORTED;
    if (batch > 65535) return PP_ERR_TOO_LARGE;
    long long first = 0;
    for (int s = 0; s < n_scales; s++) {
        if (hs[s] < 1 || ws[s] < 1) return PP_ERR_BAD_ARG;
        if ((long long)hs[s] * ws[s] > LS_MAX_PIXELS) return PP_ERR_TOO_LARGE;
        tiles->first[s] = (int)first;
        first += ((long long)hs[s] * ws[s] + LS_P - 1) / LS_P;
    }
    for (int s = n_scales; s <= LS_MAX_SCALES; s++) tiles->first[s] = (int)first;   // (<= 5 * 2^23)
    return PP_OK;
}

template <typename TP, typename TT>
void launch_terms(int mode, dim3 grid, hipStream_t st, const LossArgs &a, int stride, const void *target, long long timg, const float *mask,
                  int batch, int H, int W, int n_stacks, int n_scales, double mtw, double kpw, int flags, double *partial) {
    const TT *tg = static_cast<const TT *>(target);
    const dim3 block(LS_THREADS);
    if (mode == 0)
        hipLaunchKernelGGL((k_focal_l2<TP, TT, 0>), grid, block, 0, st, a, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw, flags,
                           partial);
    else if (mode == 1)
        hipLaunchKernelGGL((k_focal_l2<TP, TT, 1>), grid, block, 0, st, a, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw, flags,
                           partial);
    else
        hipLaunchKernelGGL((k_focal_l2<TP, TT, 2>), grid, block, 0, st, a, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw, flags,
                           partial);
}

// the argument checks both entries share, in one order (so that both refuse the same call with the same code); fills the kernel
// arguments.  f64_a / f64_b: the entry's two float64 device buffers (non-null, 8-byte aligned).  grad_dev (pp_focal_l2_grad only):
// its pointers are checked like the predictions', must differ from them, and take part in the 16-byte rule
int plan_args(const void *const *pred_dev, int pred_dtype, int pred_pixel_stride, const void *target_dev, int target_dtype,
              long long target_image_stride, const float *mask_dev, int batch, int H, int W, int n_stacks, int n_scales, const int *hs,
              const int *ws, const void *f64_a, const void *f64_b, void *const *grad_dev, LossArgs *out, GradPtrs *grads) {
    LossArgs &a = *out;
    const int rc = plan_tiles(batch, n_stacks, n_scales, hs, ws, &a.tiles);
    if (rc != PP_OK) return rc;
    if (!pred_dev || !target_dev || !f64_a || !f64_b || H < 1 || W < 1) return PP_ERR_BAD_ARG;
    if (grads && !grad_dev) return PP_ERR_BAD_ARG;
    if ((pred_dtype != PP_F16 && pred_dtype != PP_F32) || (target_dtype != PP_F16 && target_dtype != PP_F32)) return PP_ERR_BAD_ARG;
    if (pred_pixel_stride < 0 || (pred_pixel_stride > 0 && pred_pixel_stride < LS_CH)) return PP_ERR_BAD_ARG;
    if ((long long)H * W > LS_MAX_PIXELS || pred_pixel_stride > (1 << 20)) return PP_ERR_TOO_LARGE;
    if (target_image_stride < (long long)LS_CH * H * W) return PP_ERR_BAD_ARG;
    const uintptr_t pesz = pred_dtype == PP_F16 ? 2 : 4, tesz = target_dtype == PP_F16 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(target_dev) % tesz || reinterpret_cast<uintptr_t>(mask_dev) % 4 ||
        reinterpret_cast<uintptr_t>(f64_a) % 8 || reinterpret_cast<uintptr_t>(f64_b) % 8)
        return PP_ERR_BAD_ARG;
    a.vec = 0;
    for (int s = 0; s < LS_MAX_SCALES; s++) a.hs[s] = a.ws[s] = 1;
    for (int i = 0; i < LS_MAX_STACKS * LS_MAX_SCALES; i++) a.pred[i] = nullptr;
    if (grads)
        for (int i = 0; i < LS_MAX_STACKS * LS_MAX_SCALES; i++) grads->grad[i] = nullptr;
    for (int s = 0; s < n_scales; s++) {
        if (hs[s] > H || ws[s] > W) return PP_ERR_BAD_ARG;
        a.hs[s] = hs[s], a.ws[s] = ws[s];
        // 16-byte loads: every image's (and, planar, every channel's) run and every tile's start on a 16-byte boundary
        const unsigned long long hw = (unsigned long long)hs[s] * ws[s];
        const unsigned long long step = pred_pixel_stride ? hw * pred_pixel_stride : hw;   // elements between two runs' starts
        bool vec = (step * pesz) % 16 == 0 && ((unsigned long long)LS_P * (pred_pixel_stride ? pred_pixel_stride : 1) * pesz) % 16 == 0;
        for (int t = 0; t < n_stacks; t++) {
            const void *p = pred_dev[t * n_scales + s];
            if (!p || reinterpret_cast<uintptr_t>(p) % pesz) return PP_ERR_BAD_ARG;
            vec = vec && reinterpret_cast<uintptr_t>(p) % 16 == 0;
            a.pred[t * n_scales + s] = p;
            if (grads) {
                void *q = grad_dev[t * n_scales + s];
                if (!q || reinterpret_cast<uintptr_t>(q) % pesz || q == p) return PP_ERR_BAD_ARG;
                vec = vec && reinterpret_cast<uintptr_t>(q) % 16 == 0;
                grads->grad[t * n_scales + s] = q;
            }
        }
        if (vec) a.vec |= 1u << s;
    }
    if (!device_present()) return PP_ERR_NO_DEVICE;
    if ((long long)a.tiles.first[n_scales] * batch >= (1ll << 31)) return PP_ERR_TOO_LARGE;
    return PP_OK;
}

template <typename TP, typename TT>
void launch_grad(int mode, dim3 grid, hipStream_t st, const LossArgs &a, const GradPtrs &gp, int stride, const void *target, long long timg,
                 const float *mask, int batch, int H, int W, int n_stacks, int n_scales, double mtw, double kpw, int flags, const double *tw) {
    const TT *tg = static_cast<const TT *>(target);
    const dim3 block(LS_THREADS);
    if (mode == 0)
        hipLaunchKernelGGL((k_focal_l2_grad<TP, TT, 0>), grid, block, 0, st, a, gp, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw,
                           flags, tw);
    else if (mode == 1)
        hipLaunchKernelGGL((k_focal_l2_grad<TP, TT, 1>), grid, block, 0, st, a, gp, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw,
                           flags, tw);
    else
        hipLaunchKernelGGL((k_focal_l2_grad<TP, TT, 2>), grid, block, 0, st, a, gp, stride, tg, timg, mask, batch, H, W, n_stacks, n_scales, mtw, kpw,
                           flags, tw);
}

}  // namespace

extern "C" long long pp_focal_l2_workspace_bytes(int batch, int n_stacks, int n_scales, const int *hs, const int *ws) {
    LossTiles tiles;
    const int rc = plan_tiles(batch, n_stacks, n_scales, hs, ws, &tiles);
    if (rc != PP_OK) return rc;
    return (long long)batch * tiles.first[n_scales] * n_stacks * (long long)sizeof(double);
}

extern "C" int pp_focal_l2_terms(const void *const *pred_dev, int pred_dtype, int pred_pixel_stride, const void *target_dev, int target_dtype,
                                 long long target_image_stride, const float *mask_dev, int batch, int H, int W, int n_stacks, int n_scales,
                                 const int *hs, const int *ws, double multi_task_weight, double keypoint_task_weight, int flags,
                                 void *workspace_dev, double *terms_dev, void *stream) {
    LossArgs a;
    const int rc = plan_args(pred_dev, pred_dtype, pred_pixel_stride, target_dev, target_dtype, target_image_stride, mask_dev, batch, H, W, n_stacks,
                             n_scales, hs, ws, workspace_dev, terms_dev, nullptr, &a, nullptr);
    if (rc != PP_OK) return rc;
    const int tiles_per_image = a.tiles.first[n_scales];
    const dim3 grid((unsigned)((long long)tiles_per_image * batch));
    const int mode = pred_pixel_stride == 0 ? 0 : (pred_pixel_stride == 64 ? 1 : 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace_dev);
    if (pred_dtype == PP_F16 && target_dtype == PP_F16)
        launch_terms<__half, __half>(mode, grid, st, a, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks, n_scales,
                                     multi_task_weight, keypoint_task_weight, flags, partial);
    else if (pred_dtype == PP_F16)
        launch_terms<__half, float>(mode, grid, st, a, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks, n_scales,
                                    multi_task_weight, keypoint_task_weight, flags, partial);
    else if (target_dtype == PP_F16)
        launch_terms<float, __half>(mode, grid, st, a, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks, n_scales,
                                    multi_task_weight, keypoint_task_weight, flags, partial);
    else
        launch_terms<float, float>(mode, grid, st, a, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks, n_scales,
                                   multi_task_weight, keypoint_task_weight, flags, partial);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    const long long n_terms = (long long)n_stacks * n_scales * batch;
    hipLaunchKernelGGL(k_focal_l2_finish, dim3((unsigned)((n_terms + LS_THREADS - 1) / LS_THREADS)), dim3(LS_THREADS), 0, st, a.tiles,
                       static_cast<const double *>(partial), batch, n_stacks, n_scales, terms_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

extern "C" int pp_focal_l2_grad(const void *const *pred_dev, int pred_dtype, int pred_pixel_stride, const void *target_dev, int target_dtype,
                                long long target_image_stride, const float *mask_dev, int batch, int H, int W, int n_stacks, int n_scales,
                                const int *hs, const int *ws, double multi_task_weight, double keypoint_task_weight, int flags,
                                const double *term_weight_dev, void *const *grad_dev, void *stream) {
    LossArgs a;
    GradPtrs gp;
    const int rc = plan_args(pred_dev, pred_dtype, pred_pixel_stride, target_dev, target_dtype, target_image_stride, mask_dev, batch, H, W, n_stacks,
                             n_scales, hs, ws, term_weight_dev, term_weight_dev, grad_dev, &a, &gp);
    if (rc != PP_OK) return rc;
    const dim3 grid((unsigned)((long long)a.tiles.first[n_scales] * batch));
    const int mode = pred_pixel_stride == 0 ? 0 : (pred_pixel_stride == 64 ? 1 : 2);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pred_dtype == PP_F16 && target_dtype == PP_F16)
        launch_grad<__half, __half>(mode, grid, st, a, gp, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks,
                                    n_scales, multi_task_weight, keypoint_task_weight, flags, term_weight_dev);
    else if (pred_dtype == PP_F16)
        launch_grad<__half, float>(mode, grid, st, a, gp, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks,
                                   n_scales, multi_task_weight, keypoint_task_weight, flags, term_weight_dev);
    else if (target_dtype == PP_F16)
        launch_grad<float, __half>(mode, grid, st, a, gp, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks,
                                   n_scales, multi_task_weight, keypoint_task_weight, flags, term_weight_dev);
    else
        launch_grad<float, float>(mode, grid, st, a, gp, pred_pixel_stride, target_dev, target_image_stride, mask_dev, batch, H, W, n_stacks,
                                  n_scales, multi_task_weight, keypoint_task_weight, flags, term_weight_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
