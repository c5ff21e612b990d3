// posepaf_headgrad.hip -- the weight and bias gradient of a 1 x 1 convolution head (c_in -> c_out <= 64, no BN, no activation) from the
// head's binary16 pixel-major input and the binary16 gradient of its output:
//   dw[k][c] = fl32(inv_loss_scale * sum_m g[m][k] * xs[m][c]),    db[k] = fl32(inv_loss_scale * sum_m g[m][k])
//   xs[m][c] = x[m][c], or with SE gains  half_rn(float(x[m][c]) * float(scale[m / hw][c]))  (the product of two binary16 values is
//   exact in float32, so that is ONE rounding of the exact product: what pp_pw_f16 multiplies and pp_channel_scale_f16 stores)
// A reduction GEMM over the pixels; both operands are contracted along the dimension that is NOT contiguous in memory.
//
// k_head_wgrad: a persistent grid of min(HG_MAX_WG, chunks) workgroups of 256 threads; workgroup b takes the chunks of HG_P = 64
// pixels b, b + grid, b + 2 grid ... in that order.  A chunk is staged pixel-major into LDS -- the x rows with the gains applied,
// the g rows zero-filled to 64 channels (channels >= c_out are never loaded from memory: a 16-byte group that straddles c_out is
// loaded and its padding lanes are REPLACED by zero, a group wholly behind c_out is not loaded), pixels >= m as zeros -- and read
// back with ds_read_b64_tr_b16: lane l of a wave addresses row 8 (l / 32) + (l % 16) / 4, columns 16 ((l / 16) % 2) + 4 (l % 4) of a
// 16-pixel x 32-channel block and receives pixels 8 (l / 32) .. + 3 of channel l % 32, a second read 4 rows further the next four:
// the lane's share of a 32x32x16 MFMA's A (from g) and B (from x) operand, both with the pixel along K.  The reads are outside any
// divergent control flow (EXEC all ones).  Rows are padded by 64 bytes, which puts the four rows of a block on disjoint banks.
// The MFMA is v_mfma_f32_32x32x16_bf16, four per tile: v_mfma_f32_32x32x16_f16 aligns the products of a block to the exponent FIELDS
// of its operands and keeps about 25 bits below that, so a binary16 subnormal operand (exponent field 2^-14, leading zeros in the
// significand -- a few percent of a real feature map) loses up to all of its product's bits: measured 2^-18.7 relative on a
// two-pixel head, outside the contract's exact products.  Every binary16 value is EXACTLY hi + lo with hi its float32 form cut to
// 8 significant bits and lo the remaining <= 3 bits, both normal bfloat16 numbers, and a product of two bfloat16 values is exact
// in float32: acc += g_hi x_hi + g_hi x_lo + g_lo x_hi + g_lo x_lo, in this order, into the same accumulator.
// Wave w owns output rows 32 (w % 2) .. + 31 and the 32-column tiles w / 2, w / 2 + 2, ... (c_in / 64 of them: 64 accumulator
// registers per lane at c_in = 256).  The next chunk's global loads are issued into registers before the current chunk's MFMAs.
// The bias sums come from the same LDS image: thread (k = tid % 64, q = tid / 64) adds pixels 16 q .. 16 q + 15 of channel k in
// order; the four quarters are added in order at the end.  Every workgroup stores its c_out x c_in + c_out float32 partials with
// plain stores; k_head_wgrad_finish adds the workgroups' partials of one element (four interleaved runs in workgroup order, then
// ((s0 + s1) + s2) + s3), multiplies by inv_loss_scale once and stores dw / db.  No atomics, nothing is assumed zero: the order of
// the additions follows from (m, c_in, c_out) alone.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "posepaf_headgrad.h"      // the accumulate pass and its pieces, shared with posepaf_convgrad.hip
#include "posepaf_internal.h"

namespace {

template <int C_IN, bool GVEC>
__global__ __launch_bounds__(HG_THREADS) void k_head_wgrad(const __half *__restrict__ g, int ldg, const __half *__restrict__ x,
                                                            const __half *__restrict__ scale, long long m, int hw, int c_out,
                                                            int n_chunks, float *__restrict__ partial) {
    head_wgrad_accumulate<C_IN, GVEC>(g, ldg, x, scale, m, hw, c_out, n_chunks, (int)gridDim.x, (int)blockIdx.x, partial, SamePixel{});
}

// elements 64 block .. + 63 of (dw, db): the workgroups' partials in four interleaved runs, each in workgroup order, then the four in order
__device__ __forceinline__ void head_wgrad_finish(const float *__restrict__ partial, int n_wg, int n_dw, int n_db, float inv_loss_scale,
                                                  float *__restrict__ dw, float *__restrict__ db, int block) {
    __shared__ float s_sum[HG_THREADS];
    const int tid = threadIdx.x, q = tid >> 6;
    const int e = block * 64 + (tid & 63), n = n_dw + n_db;
    float sum = 0.0f;
    if (e < n)
        for (int w = q; w < n_wg; w += 4) sum += partial[(size_t)w * n + e];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid < 64 && e < n) {
        const float v = (((s_sum[tid] + s_sum[64 + tid]) + s_sum[128 + tid]) + s_sum[192 + tid]) * inv_loss_scale;
        if (e < n_dw) dw[e] = v;
        else db[e - n_dw] = v;
    }
}

__global__ __launch_bounds__(HG_THREADS) void k_head_wgrad_finish(const float *__restrict__ partial, int n_wg, int n_dw, int n_db,
                                                                   float inv_loss_scale, float *__restrict__ dw, float *__restrict__ db) {
    head_wgrad_finish(partial, n_wg, n_dw, n_db, inv_loss_scale, dw, db, (int)blockIdx.x);
}

// ---- every head of a step in one call: the tables travel by value in the kernel arguments (a graph capture freezes them).
// first[i] is the first workgroup of head i of this launch, first[n] the grid; a workgroup finds its head by walking the table.
struct MultiHead {
    const __half *g, *x, *scale;
    float *partial;
    long long m;
    int ldg, hw, c_out, n_chunks, grid;
};

struct MultiAccumulate {
    MultiHead head[PP_HEAD_WGRAD_MULTI_MAX];
    int first[PP_HEAD_WGRAD_MULTI_MAX + 1];
    int n;
};

struct MultiFinishHead {
    const float *partial;
    float *dw, *db;
    int n_wg, n_dw, n_db;
};

struct MultiFinish {
    MultiFinishHead head[PP_HEAD_WGRAD_MULTI_MAX];
    int first[PP_HEAD_WGRAD_MULTI_MAX + 1];
    int n;
};

static_assert(sizeof(MultiAccumulate) <= 4096 && sizeof(MultiFinish) + 16 <= 4096, "the tables must fit the kernel arguments");

template <int C_IN, bool GVEC>
__global__ __launch_bounds__(HG_THREADS) void k_head_wgrad_multi(const MultiAccumulate t) {
    const int b = (int)blockIdx.x;
    int i = 0;
    while (i + 1 < t.n && b >= t.first[i + 1]) i++;      // uniform over the workgroup
    const MultiHead &h = t.head[i];
    head_wgrad_accumulate<C_IN, GVEC>(h.g, h.ldg, h.x, h.scale, h.m, h.hw, h.c_out, h.n_chunks, h.grid, b - t.first[i], h.partial, SamePixel{});
}

// inv_dev: the factor on the device (a captured step whose loss scale moves), else the host's
__global__ __launch_bounds__(HG_THREADS) void k_head_wgrad_multi_finish(const MultiFinish t, float inv_loss_scale, const float *__restrict__ inv_dev) {
    const int b = (int)blockIdx.x;
    int i = 0;
    while (i + 1 < t.n && b >= t.first[i + 1]) i++;
    const MultiFinishHead &h = t.head[i];
    head_wgrad_finish(h.partial, h.n_wg, h.n_dw, h.n_db, inv_dev ? *inv_dev : inv_loss_scale, h.dw, h.db, b - t.first[i]);
}

int grid_of(long long m) {
    const long long c = n_chunks_of(m);
    return (int)(c < HG_MAX_WG ? c : HG_MAX_WG);
}

template <int C_IN>
void launch(bool gvec, int grid, hipStream_t st, const __half *g, int ldg, const __half *x, const __half *scale, long long m, int hw,
            int c_out, int n_chunks, float *partial) {
    if (gvec)
        hipLaunchKernelGGL((k_head_wgrad<C_IN, true>), dim3(grid), dim3(HG_THREADS), 0, st, g, ldg, x, scale, m, hw, c_out, n_chunks, partial);
    else
        hipLaunchKernelGGL((k_head_wgrad<C_IN, false>), dim3(grid), dim3(HG_THREADS), 0, st, g, ldg, x, scale, m, hw, c_out, n_chunks, partial);
}

}  // namespace

extern "C" int pp_head_wgrad_supported(int c_in, int c_out) {
    return (c_in >= 64 && c_in <= 256 && c_in % 64 == 0 && c_out >= 1 && c_out <= HG_KP) ? 1 : 0;
}

extern "C" int pp_head_wgrad_chunk_pixels(void) { return HG_P; }

extern "C" int pp_head_wgrad_max_workgroups(void) { return HG_MAX_WG; }

extern "C" long long pp_head_wgrad_workspace_bytes(long m, int c_in, int c_out) {
    if (m <= 0) return PP_ERR_BAD_ARG;
    if (!pp_head_wgrad_supported(c_in, c_out)) return PP_ERR_UNSUPPORTED;
    if ((long long)m > 2147483647ll) return PP_ERR_TOO_LARGE;
    return (long long)grid_of(m) * ((long long)c_out * c_in + c_out) * (long long)sizeof(float);
}

namespace {

// THE list of refusals of one head, in the documented order; both entries go through it.  own_workspace / own_factor: the single
// entry's workspace and host factor, tested where its list has them; the multi entry passes neither (it tests its one workspace
// and its factor after every head).  The workspace SIZE comes after this list in both entries.
int check_head(const pp_head_wgrad_desc &h, void *const *own_workspace, const float *own_factor) {
    if (!h.g || !h.x || !h.dw || !h.db || (own_workspace && !*own_workspace)) return PP_ERR_BAD_ARG;
    if (h.m <= 0 || h.hw <= 0 || (h.scale && h.m % h.hw != 0)) return PP_ERR_BAD_ARG;
    if (h.c_out > 0 && h.ldg < h.c_out) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(h.x) % 16 || reinterpret_cast<uintptr_t>(h.scale) % 16 || reinterpret_cast<uintptr_t>(h.g) % 2 ||
        reinterpret_cast<uintptr_t>(h.dw) % 4 || reinterpret_cast<uintptr_t>(h.db) % 4 ||
        (own_workspace && reinterpret_cast<uintptr_t>(*own_workspace) % 4))
        return PP_ERR_BAD_ARG;
    if (own_factor && !(isfinite(*own_factor) && *own_factor > 0.0f)) return PP_ERR_BAD_ARG;
    if (!pp_head_wgrad_supported(h.c_in, h.c_out) || (h.scale && h.hw % 64 != 0)) return PP_ERR_UNSUPPORTED;
    if ((long long)h.m > 2147483647ll) return PP_ERR_TOO_LARGE;
    return PP_OK;
}

}  // namespace

extern "C" int pp_head_wgrad_f16(const void *g, int ldg, const void *x, const void *scale, long m, int hw, int c_in, int c_out,
                                 float inv_loss_scale, void *workspace, long long workspace_bytes, float *dw, float *db, void *stream) {
    const pp_head_wgrad_desc h = {g, ldg, x, scale, m, hw, c_in, c_out, dw, db};
    const int rc = check_head(h, &workspace, &inv_loss_scale);
    if (rc != PP_OK) return rc;
    if (workspace_bytes < pp_head_wgrad_workspace_bytes(m, c_in, c_out)) return PP_ERR_BAD_ARG;
    if (!device_present()) return PP_ERR_NO_DEVICE;

    const int n_chunks = (int)n_chunks_of(m), grid = grid_of(m);
    const bool gvec = reinterpret_cast<uintptr_t>(g) % 16 == 0 && ldg % 8 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __half *gh = static_cast<const __half *>(g), *xh = static_cast<const __half *>(x), *sh = static_cast<const __half *>(scale);
    float *partial = static_cast<float *>(workspace);
    switch (c_in) {
        case 64: launch<64>(gvec, grid, st, gh, ldg, xh, sh, m, hw, c_out, n_chunks, partial); break;
        case 128: launch<128>(gvec, grid, st, gh, ldg, xh, sh, m, hw, c_out, n_chunks, partial); break;
        case 192: launch<192>(gvec, grid, st, gh, ldg, xh, sh, m, hw, c_out, n_chunks, partial); break;
        default: launch<256>(gvec, grid, st, gh, ldg, xh, sh, m, hw, c_out, n_chunks, partial); break;
    }
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    const int n_dw = c_out * c_in, n = n_dw + c_out;
    hipLaunchKernelGGL(k_head_wgrad_finish, dim3((n + 63) / 64), dim3(HG_THREADS), 0, st, static_cast<const float *>(partial), grid, n_dw, c_out,
                       inv_loss_scale, dw, db);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

namespace {

int check_table(int n_heads, const pp_head_wgrad_desc *heads) {
    if (!heads || n_heads <= 0) return PP_ERR_BAD_ARG;
    if (n_heads > PP_HEAD_WGRAD_MULTI_MAX) return PP_ERR_UNSUPPORTED;
    for (int i = 0; i < n_heads; i++) {
        const int rc = check_head(heads[i], nullptr, nullptr);
        if (rc != PP_OK) return rc;
    }
    return PP_OK;
}

bool gvec_of(const pp_head_wgrad_desc &h) { return reinterpret_cast<uintptr_t>(h.g) % 16 == 0 && h.ldg % 8 == 0; }

template <int C_IN>
void launch_multi(bool gvec, hipStream_t st, const MultiAccumulate &t) {
    const int grid = t.first[t.n];
    if (gvec) hipLaunchKernelGGL((k_head_wgrad_multi<C_IN, true>), dim3(grid), dim3(HG_THREADS), 0, st, t);
    else hipLaunchKernelGGL((k_head_wgrad_multi<C_IN, false>), dim3(grid), dim3(HG_THREADS), 0, st, t);
}

}  // namespace

extern "C" int pp_head_wgrad_multi_max_heads(void) { return PP_HEAD_WGRAD_MULTI_MAX; }

extern "C" long long pp_head_wgrad_multi_workspace_bytes(int n_heads, const pp_head_wgrad_desc *heads) {
    const int rc = check_table(n_heads, heads);
    if (rc != PP_OK) return rc;
    long long total = 0;
    for (int i = 0; i < n_heads; i++) total += pp_head_wgrad_workspace_bytes(heads[i].m, heads[i].c_in, heads[i].c_out);   // multiples of 4
    return total;
}

extern "C" int pp_head_wgrad_multi_f16(int n_heads, const pp_head_wgrad_desc *heads, float inv_loss_scale, const float *inv_loss_scale_dev,
                                       void *workspace, long long workspace_bytes, void *stream) {
    const long long need = pp_head_wgrad_multi_workspace_bytes(n_heads, heads);
    if (need < 0) return (int)need;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 4 || workspace_bytes < need) return PP_ERR_BAD_ARG;
    if (inv_loss_scale_dev ? reinterpret_cast<uintptr_t>(inv_loss_scale_dev) % 4 != 0 : !(isfinite(inv_loss_scale) && inv_loss_scale > 0.0f))
        return PP_ERR_BAD_ARG;
    if (!device_present()) return PP_ERR_NO_DEVICE;

    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial[PP_HEAD_WGRAD_MULTI_MAX];
    char *at = static_cast<char *>(workspace);
    for (int i = 0; i < n_heads; i++) {
        partial[i] = reinterpret_cast<float *>(at);
        at += pp_head_wgrad_workspace_bytes(heads[i].m, heads[i].c_in, heads[i].c_out);
    }
    // one accumulate launch per (c_in, load form) among the heads, in the order of their first appearance
    bool done[PP_HEAD_WGRAD_MULTI_MAX] = {};
    for (int i = 0; i < n_heads; i++) {
        if (done[i]) continue;
        const int c_in = heads[i].c_in;
        const bool gvec = gvec_of(heads[i]);
        MultiAccumulate t;
        t.n = 0, t.first[0] = 0;
        for (int j = i; j < n_heads; j++) {
            const pp_head_wgrad_desc &h = heads[j];
            if (done[j] || h.c_in != c_in || gvec_of(h) != gvec) continue;
            done[j] = true;
            MultiHead &d = t.head[t.n];
            d.g = static_cast<const __half *>(h.g), d.x = static_cast<const __half *>(h.x), d.scale = static_cast<const __half *>(h.scale);
            d.partial = partial[j], d.m = h.m, d.ldg = h.ldg, d.hw = h.hw, d.c_out = h.c_out;
            d.n_chunks = (int)n_chunks_of(h.m), d.grid = grid_of(h.m);
            t.first[t.n + 1] = t.first[t.n] + d.grid;
            t.n++;
        }
        switch (c_in) {
            case 64: launch_multi<64>(gvec, st, t); break;
            case 128: launch_multi<128>(gvec, st, t); break;
            case 192: launch_multi<192>(gvec, st, t); break;
            default: launch_multi<256>(gvec, st, t); break;
        }
        if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    }
    MultiFinish f;
    f.n = n_heads, f.first[0] = 0;
    for (int i = 0; i < n_heads; i++) {
        const pp_head_wgrad_desc &h = heads[i];
        MultiFinishHead &d = f.head[i];
        d.partial = partial[i], d.dw = h.dw, d.db = h.db, d.n_wg = grid_of(h.m), d.n_dw = h.c_out * h.c_in, d.n_db = h.c_out;
        f.first[i + 1] = f.first[i] + (d.n_dw + d.n_db + 63) / 64;
    }
    hipLaunchKernelGGL(k_head_wgrad_multi_finish, dim3(f.first[n_heads]), dim3(HG_THREADS), 0, st, f, inv_loss_scale, inv_loss_scale_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
