// posepaf_convgrad.hip -- one layer below the heads (include/posepaf.h): the gradient through a 1 x 1 head and the LeakyReLU in
// front of it, and the weight and bias gradient of the 3 x 3 / pad 1 / stride 1 convolution that feeds that activation.
//
// k_head_dgrad:  dx[m][c] = half_rn(t),  t = s where y[m][c] > 0 else fl32(slope * s),  s = sum_k g[m][k] * w[k][c].
//   An HBM stream (g and y read once, dx written once) with c_out multiply-adds per element, on the vector ALU: a binary16 value is
//   exact in float32 and so is the product of two of them (22 significant bits, exponent >= 2^-48), so fmaf(float(g), float(w), acc)
//   IS acc + the exact product rounded once -- the contract, subnormals included, with no operand split (the split of
//   posepaf_headgrad.hip repairs the binary16 MFMA, which is not used here).  A persistent grid of min(512, chunks) workgroups of
//   256 threads; w is staged once per workgroup as binary16 (c_out x c_in), a chunk of 64 pixels of g as float32 with channels at or
//   behind c_out as zeros (never loaded).  A wave takes (64 columns, 16 pixels) items: lane l keeps column c's c_out weights in
//   registers, reads a pixel's g as LDS broadcasts and adds k = 0, 1, ... c_out - 1 in this order into one accumulator per pixel
//   (the zero products of a last partial group of four add nothing).  |dx - exact| <= E + max(2^-11 (|t| + E), 2^-25) with
//   E = a 2^-24 (c_out sum_k |g w| + |s|), a = 1 or slope: c_out float32 additions, one float32 multiply, one binary16 rounding.
//
// k_conv3x3_wgrad: the reduction GEMM of posepaf_headgrad.h once per sub-problem (tap (r, s), 64 output channels): g is dy's 64-channel
//   slice with row pitch c_out, and the x row of pixel p is the row of its neighbour (r - 1, s - 1) in the same image -- or zeros,
//   without a load, where that lies outside.  Sub-problem j = 9 (k / 64) + 3 r + s owns workgroups j * grid .. + grid - 1 of ONE launch,
//   grid = min(CG_MAX_WG, chunks), each with the chunks wg, wg + grid, ... of the head kernel's pipeline and its 64 x c_in + 64 partials.
//   k_conv3x3_wgrad_finish adds an element's partials as the head's finish does (four interleaved runs in workgroup order, then
//   ((s0 + s1) + s2) + s3), multiplies by the factor once and stores dw in (c_out, 3, 3, c_in) order; db comes from the centre tap's
//   sub-problems.  No atomics, nothing assumed zero: (n, h, w, c_in, c_out) fixes the order of every addition.
//
// k_conv3x3_dgrad: dx[b, i, j, c] = half_rn(t),  t = s where y > 0 (or y == NULL) else fl32(slope * s),
//   s = sum over (r, q, k) with (i + 1 - r, j + 1 - q) inside image b of dy[b, i + 1 - r, j + 1 - q, k] * w[k][r][q][c].
//   An implicit GEMM on the matrix unit: c_in x 64 pixels per workgroup (an 8 x 8 tile of one image), reduction 9 c_out, all of it in
//   this workgroup.  The dy halo tile (10 x 10 pixels, zeros -- staged without a load -- where outside the image) goes to LDS ONCE
//   for all nine taps, already split into bfloat16 hi and lo images (split_bf16: hi + lo is the binary16 value exactly), so the
//   pixel operand of every MFMA is one 16-byte LDS read.  The weights stream per (tap, 32 output channels) through registers into a
//   double-buffered LDS image of 32 rows of w -- rows of a fixed tap are contiguous in c, the read is the transposed one of
//   posepaf_headgrad.h -- and are split once per read (each weight element is read by two waves, one per half of the pixels).  Four
//   mfma_f32_32x32x16_bf16 per operand pair (hi hi, hi lo, lo hi, lo lo) make every product exact.  A wave owns 32 pixels and
//   c_in / 64 tiles of 32 channels; the loop runs tap 0 .. 8, k 0 .. c_out - 1 in this order.  The epilogue reads y and stores dx as
//   8-byte groups of four channels.  No atomics, no workspace: (n, h, w, c_in, c_out) fixes the order of every addition.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include <atomic>

#include "posepaf_headgrad.h"
#include "posepaf_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------ the head's data gradient

constexpr int DG_THREADS = 256;
constexpr int DG_P = 64;              // pixels of a chunk
constexpr int DG_MAX_WG = 512;        // two workgroups per CU
constexpr int DG_K = 64;              // the largest c_out

template <int C_IN>
__global__ __launch_bounds__(DG_THREADS) void k_head_dgrad(const __half *__restrict__ g, int ldg, const __half *__restrict__ w,
                                                            const __half *__restrict__ y, long long m, int c_out, float slope, int n_chunks,
                                                            __half *__restrict__ dx) {
    constexpr int NCG = C_IN / 64;                    // 64-column groups
    constexpr int ITEMS = NCG * 4;                    // (column group, 16 pixels) of a chunk

    __shared__ alignas(16) __half s_w[DG_K * C_IN];   // rows >= c_out are never written or read
    __shared__ alignas(16) float s_g[DG_P * DG_K];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int v = tid; v < c_out * (C_IN / 8); v += DG_THREADS)
        reinterpret_cast<Quad *>(s_w)[v] = reinterpret_cast<const Quad *>(w)[v];

    const unsigned short *gs = reinterpret_cast<const unsigned short *>(g);
    for (int chunk = (int)blockIdx.x; chunk < n_chunks; chunk += (int)gridDim.x) {
        const long long p0 = (long long)chunk * DG_P;
        __syncthreads();                              // the previous chunk's reads of s_g are done
#pragma unroll
        for (int i = 0; i < DG_P * DG_K / DG_THREADS; i++) {
            const int e = tid + DG_THREADS * i, pix = e >> 6, k = e & 63;
            unsigned short bits = 0;
            if (p0 + pix < m && k < c_out) bits = gs[(size_t)(p0 + pix) * ldg + k];
            s_g[e] = __half2float(__ushort_as_half(bits));
        }
        __syncthreads();                              // (the first pass: s_w as well)

        for (int item = wave; item < ITEMS; item += 4) {
            const int c = 64 * (item % NCG) + lane, pix0 = 16 * (item / NCG);
            unsigned short yv[16];
#pragma unroll
            for (int p = 0; p < 16; p++) {
                yv[p] = 0;
                if (p0 + pix0 + p < m) yv[p] = reinterpret_cast<const unsigned short *>(y)[(size_t)(p0 + pix0 + p) * C_IN + c];
            }
            float wcol[DG_K], acc[16];
#pragma unroll
            for (int k = 0; k < DG_K; k++) wcol[k] = k < c_out ? __half2float(s_w[k * C_IN + c]) : 0.0f;
#pragma unroll
            for (int p = 0; p < 16; p++) acc[p] = 0.0f;
#pragma unroll
            for (int k4 = 0; k4 < DG_K / 4; k4++) {
                if (4 * k4 < c_out) {                 // uniform
#pragma unroll
                    for (int p = 0; p < 16; p++) {
                        const float4 gv = *reinterpret_cast<const float4 *>(s_g + (pix0 + p) * DG_K + 4 * k4);
                        acc[p] = __fmaf_rn(gv.x, wcol[4 * k4 + 0], acc[p]);
                        acc[p] = __fmaf_rn(gv.y, wcol[4 * k4 + 1], acc[p]);
                        acc[p] = __fmaf_rn(gv.z, wcol[4 * k4 + 2], acc[p]);
                        acc[p] = __fmaf_rn(gv.w, wcol[4 * k4 + 3], acc[p]);
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < 16; p++) {
                if (p0 + pix0 + p < m) {
                    const bool pass = __half2float(__ushort_as_half(yv[p])) > 0.0f;      // +-0 and every negative value: the slope
                    const float t = pass ? acc[p] : __fmul_rn(slope, acc[p]);
                    dx[(size_t)(p0 + pix0 + p) * C_IN + c] = __float2half_rn(t);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 weight gradient

constexpr int CG_MAX_WG = 16;         // workgroups of one sub-problem: 36 sub-problems at 256 -> 256 fill the device twice over

int conv_grid_of(long long m) {
    const long long c = n_chunks_of(m);
    return (int)(c < CG_MAX_WG ? c : CG_MAX_WG);
}

template <int C_IN>
__global__ __launch_bounds__(HG_THREADS) void k_conv3x3_wgrad(const __half *__restrict__ dy, const __half *__restrict__ x, long long m, int h,
                                                               int w, int c_out, int n_chunks, int grid, float *__restrict__ partial) {
    const int sub = (int)blockIdx.x / grid, wg = (int)blockIdx.x - sub * grid;      // uniform over the workgroup
    const int tap = sub % 9, slice = sub / 9;
    head_wgrad_accumulate<C_IN, true>(dy + 64 * slice, c_out, x, nullptr, m, 1, HG_KP, n_chunks, grid, wg,
                                      partial + (size_t)sub * grid * ((size_t)HG_KP * C_IN + HG_KP), TapPixel{h, w, tap / 3 - 1, tap % 3 - 1});
}

// block b < c_out 9 c_in / 64: elements 64 b .. + 63 of dw (one output channel, one tap, 64 input channels); the blocks behind: 64 of db
__global__ __launch_bounds__(HG_THREADS) void k_conv3x3_wgrad_finish(const float *__restrict__ partial, int grid, int c_in, int c_out,
                                                                      float inv_loss_scale, const float *__restrict__ inv_dev,
                                                                      float *__restrict__ dw, float *__restrict__ db) {
    __shared__ float s_sum[HG_THREADS];
    const int tid = threadIdx.x, q = tid >> 6, l = tid & 63, b = (int)blockIdx.x;
    const int n_dw_blocks = c_out * 9 * (c_in / 64);
    const size_t per = (size_t)HG_KP * c_in + HG_KP;
    int sub, off;
    if (b < n_dw_blocks) {
        const int e = b * 64 + l, k = e / (9 * c_in), rem = e - k * 9 * c_in, tap = rem / c_in;
        sub = 9 * (k >> 6) + tap, off = (k & 63) * c_in + (rem - tap * c_in);
    } else {
        const int k = (b - n_dw_blocks) * 64 + l;
        sub = 9 * (k >> 6) + 4, off = HG_KP * c_in + (k & 63);
    }
    const float *src = partial + (size_t)sub * grid * per + off;
    float sum = 0.0f;
    for (int wg = q; wg < grid; wg += 4) sum += src[(size_t)wg * per];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid < 64) {
        const float v = (((s_sum[tid] + s_sum[64 + tid]) + s_sum[128 + tid]) + s_sum[192 + tid]) * (inv_dev ? *inv_dev : inv_loss_scale);
        if (b < n_dw_blocks) dw[(size_t)b * 64 + l] = v;
        else db[(b - n_dw_blocks) * 64 + l] = v;
    }
}

// ------------------------------------------------------------------------------------------------ the 3 x 3 data gradient

constexpr int CD_THREADS = 256;
constexpr int CD_T = 8;                           // the tile is CD_T x CD_T pixels
constexpr int CD_HALO = CD_T + 2;
constexpr int CD_HP = CD_HALO * CD_HALO;          // pixels of the dy halo tile
constexpr int CD_KS = 32;                         // output channels (rows of w) of a weight slice
constexpr int CD_PADK = 8;                        // bfloat16 elements of padding behind a halo pixel's row (16 bytes)

constexpr int conv_dgrad_lds_bytes(int c_in, int c_out) {
    return 2 * CD_HP * (c_out + CD_PADK) * 2 + 2 * CD_KS * (c_in + HG_PAD) * 2;
}

template <int C_IN>
__global__ __launch_bounds__(CD_THREADS) void k_conv3x3_dgrad(const __half *__restrict__ dy, const __half *__restrict__ w,
                                                               const __half *__restrict__ y, int h, int wd, int c_out, int tiles_x, int tiles_y,
                                                               float slope, __half *__restrict__ dx) {
    constexpr int WROW = C_IN + HG_PAD;
    constexpr int VPR = C_IN / 8;                     // 16-byte groups of a row of w
    constexpr int NV = CD_KS * VPR / CD_THREADS;      // groups of a thread and slice
    constexpr int NB = C_IN / 64;                     // 32-channel tiles of a wave

    extern __shared__ __align__(16) unsigned char smem[];
    const int SD = c_out + CD_PADK;
    unsigned short *s_hi = reinterpret_cast<unsigned short *>(smem), *s_lo = s_hi + CD_HP * SD;
    __half *s_w = reinterpret_cast<__half *>(s_lo + CD_HP * SD);      // [2][CD_KS * WROW]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned bid = blockIdx.x, tq = bid / (unsigned)tiles_x;
    const int j0 = CD_T * (int)(bid - tq * (unsigned)tiles_x), i0 = CD_T * (int)(tq % (unsigned)tiles_y);
    const size_t img_row0 = (size_t)(tq / (unsigned)tiles_y) * (size_t)h;        // the first row of this image, counted over the batch

    // a thread's NV 16-byte groups of the next slice, held in named registers across the MFMA block (an indexed array of them is
    // not promoted to registers here and lands in scratch)
    uint4 wr0 = {}, wr1 = {}, wr2 = {}, wr3 = {};
    static_assert(NV >= 1 && NV <= 4, "wr0 .. wr3");
    auto load_slice = [&](int it) __attribute__((always_inline)) {
        const int slices = c_out / CD_KS, tap = it / slices, k0 = CD_KS * (it - tap * slices);
        auto src = [&](int i) {
            const int v = tid + CD_THREADS * i, row = v / VPR, cv = v - row * VPR;
            return reinterpret_cast<const uint4 *>(w + ((size_t)(k0 + row) * 9 + tap) * C_IN + cv * 8);
        };
        wr0 = *src(0);
        if constexpr (NV > 1) wr1 = *src(1);
        if constexpr (NV > 2) wr2 = *src(2);
        if constexpr (NV > 3) wr3 = *src(3);
    };
    auto stage_slice = [&](int buf) __attribute__((always_inline)) {
        auto dst = [&](int i) {
            const int v = tid + CD_THREADS * i, row = v / VPR, cv = v - row * VPR;
            return reinterpret_cast<uint4 *>(s_w + buf * (CD_KS * WROW) + row * WROW + cv * 8);
        };
        *dst(0) = wr0;
        if constexpr (NV > 1) *dst(1) = wr1;
        if constexpr (NV > 2) *dst(2) = wr2;
        if constexpr (NV > 3) *dst(3) = wr3;
    };

    load_slice(0);
    // the dy halo tile, once: a pixel outside the image is zeros and is not loaded
    const int vpp = c_out / 8;
    for (int v = tid; v < CD_HP * vpp; v += CD_THREADS) {
        const int pix = v / vpp, cv = v - pix * vpp, hi_ = pix / CD_HALO;
        const int ii = i0 + hi_ - 1, jj = j0 + (pix - hi_ * CD_HALO) - 1;
        half8v val = {0, 0, 0, 0, 0, 0, 0, 0};
        if ((unsigned)ii < (unsigned)h && (unsigned)jj < (unsigned)wd)
            val = *reinterpret_cast<const half8v *>(dy + ((img_row0 + ii) * (size_t)wd + jj) * c_out + cv * 8);
        bf8v vh, vl;
        split_bf16(val, vh, vl);
        *reinterpret_cast<bf8v *>(s_hi + pix * SD + cv * 8) = vh;
        *reinterpret_cast<bf8v *>(s_lo + pix * SD + cv * 8) = vl;
    }
    stage_slice(0);
    __syncthreads();

    float16v acc[NB];
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;

    const int ptile = wave & 1, mt0 = wave >> 1;
    const int pl = 32 * ptile + (lane & 31), pi = pl >> 3, pj = pl & 7;      // this lane's pixel of the tile
    const int n_it = 9 * (c_out / CD_KS);
    for (int it = 0; it < n_it; it++) {
        const int slices = c_out / CD_KS, tap = it / slices, k0 = CD_KS * (it - tap * slices);
        const int r = tap / 3, q = tap - 3 * r;
        if (it + 1 < n_it) load_slice(it + 1);
        const __half *wimg = s_w + (it & 1) * (CD_KS * WROW);
        const int drow = ((pi + 2 - r) * CD_HALO + (pj + 2 - q)) * SD + k0 + 8 * (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < CD_KS / 16; kk++) {
            const bf8v b_hi = *reinterpret_cast<const bf8v *>(s_hi + drow + 16 * kk);
            const bf8v b_lo = *reinterpret_cast<const bf8v *>(s_lo + drow + 16 * kk);
#pragma unroll
            for (int j = 0; j < NB; j++) {
                bf8v a_hi, a_lo;
                split_bf16(tr_frag(wimg, WROW, 16 * kk, 32 * (mt0 + 2 * j), lane), a_hi, a_lo);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_lo, acc[j], 0, 0, 0);
            }
        }
        if (it + 1 < n_it) stage_slice((it + 1) & 1);     // the buffer iteration it - 1 read: every wave passed the barrier behind it
        __syncthreads();
    }

    // acc[j][reg]: pixel pl, channel 32 (mt0 + 2 j) + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int gi = i0 + pi, gj = j0 + pj;
    if (gi < h && gj < wd) {
        const size_t base = ((img_row0 + gi) * (size_t)wd + gj) * C_IN;
#pragma unroll
        for (int j = 0; j < NB; j++) {
#pragma unroll
            for (int rg = 0; rg < 4; rg++) {
                const int c0 = 32 * (mt0 + 2 * j) + 8 * rg + 4 * (lane >> 5);
                uint2 yv = make_uint2(0x3c003c00u, 0x3c003c00u);      // y == NULL: every element passes
                if (y) yv = *reinterpret_cast<const uint2 *>(y + base + c0);
                // y > 0 as a test of the binary16 bits: sign clear, not zero, not a NaN (a NaN fails y > 0 and takes the slope)
                auto one = [&](float s, unsigned yb) {
                    const bool pass = yb - 1u < 0x7c00u;
                    return (unsigned)__half_as_ushort(__float2half_rn(pass ? s : __fmul_rn(slope, s)));
                };
                const unsigned o0 = one(acc[j][4 * rg + 0], yv.x & 0xffffu), o1 = one(acc[j][4 * rg + 1], yv.x >> 16);
                const unsigned o2 = one(acc[j][4 * rg + 2], yv.y & 0xffffu), o3 = one(acc[j][4 * rg + 3], yv.y >> 16);
                *reinterpret_cast<uint2 *>(dx + base + c0) = make_uint2(o0 | (o1 << 16), o2 | (o3 << 16));
            }
        }
    }
}

// The kernel's LDS exceeds the 64 KiB default, so its limit is raised once per DEVICE and instance (a process may hold several
// GPUs; the flags are atomic, and two threads that both find one clear set the same value twice).  Never inside a stream capture:
// a first call there is refused with PP_ERR_UNSUPPORTED, as posepaf_conv_own.hip's ensure_attr does -- call once eagerly first.
constexpr int CD_MAX_DEVICES = 32;

template <int C_IN>
int launch_conv_dgrad(unsigned blocks, hipStream_t st, const __half *dy, const __half *w, const __half *y, int h, int wd, int c_out,
                      int tiles_x, int tiles_y, float slope, __half *dx) {
    static std::atomic<bool> attr_set[CD_MAX_DEVICES];        // zero-initialised
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= CD_MAX_DEVICES) return PP_ERR_HIP;
    if (!attr_set[dev].load(std::memory_order_acquire)) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) return PP_ERR_HIP;
        if (cs != hipStreamCaptureStatusNone) return PP_ERR_UNSUPPORTED;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_conv3x3_dgrad<C_IN>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                conv_dgrad_lds_bytes(C_IN, 256)) != hipSuccess)
            return PP_ERR_HIP;
        attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL((k_conv3x3_dgrad<C_IN>), dim3(blocks), dim3(CD_THREADS), conv_dgrad_lds_bytes(C_IN, c_out), st, dy, w, y, h, wd, c_out,
                       tiles_x, tiles_y, slope, dx);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

template <int C_IN>
void launch_dgrad(int grid, hipStream_t st, const __half *g, int ldg, const __half *w, const __half *y, long long m, int c_out, float slope,
                  int n_chunks, __half *dx) {
    hipLaunchKernelGGL((k_head_dgrad<C_IN>), dim3(grid), dim3(DG_THREADS), 0, st, g, ldg, w, y, m, c_out, slope, n_chunks, dx);
}

template <int C_IN>
void launch_conv(int blocks, hipStream_t st, const __half *dy, const __half *x, long long m, int h, int w, int c_out, int n_chunks, int grid,
                 float *partial) {
    hipLaunchKernelGGL((k_conv3x3_wgrad<C_IN>), dim3(blocks), dim3(HG_THREADS), 0, st, dy, x, m, h, w, c_out, n_chunks, grid, partial);
}

}  // namespace

extern "C" int pp_head_dgrad_supported(int c_in, int c_out) {
    return (c_in >= 64 && c_in <= 256 && c_in % 64 == 0 && c_out >= 1 && c_out <= DG_K) ? 1 : 0;
}

extern "C" int pp_head_dgrad_f16(const void *g, int ldg, const void *w, const void *y, long m, int c_in, int c_out, float slope, void *dx,
                                 void *stream) {
    if (!g || !w || !y || !dx) return PP_ERR_BAD_ARG;
    if (m <= 0) return PP_ERR_BAD_ARG;
    if (c_out > 0 && ldg < c_out) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(g) % 2 || reinterpret_cast<uintptr_t>(w) % 16 || reinterpret_cast<uintptr_t>(y) % 16 ||
        reinterpret_cast<uintptr_t>(dx) % 16)
        return PP_ERR_BAD_ARG;
    if (!(isfinite(slope) && slope > 0.0f)) return PP_ERR_BAD_ARG;
    if (!pp_head_dgrad_supported(c_in, c_out)) return PP_ERR_UNSUPPORTED;
    if ((long long)m > 2147483647ll) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;

    const long long chunks = (m + DG_P - 1) / DG_P;
    const int n_chunks = (int)chunks, grid = (int)(chunks < DG_MAX_WG ? chunks : DG_MAX_WG);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __half *gh = static_cast<const __half *>(g), *wh = static_cast<const __half *>(w), *yh = static_cast<const __half *>(y);
    __half *dh = static_cast<__half *>(dx);
    switch (c_in) {
        case 64: launch_dgrad<64>(grid, st, gh, ldg, wh, yh, m, c_out, slope, n_chunks, dh); break;
        case 128: launch_dgrad<128>(grid, st, gh, ldg, wh, yh, m, c_out, slope, n_chunks, dh); break;
        case 192: launch_dgrad<192>(grid, st, gh, ldg, wh, yh, m, c_out, slope, n_chunks, dh); break;
        default: launch_dgrad<256>(grid, st, gh, ldg, wh, yh, m, c_out, slope, n_chunks, dh); break;
    }
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

extern "C" int pp_conv3x3_wgrad_supported(int c_in, int c_out) {
    return (c_in >= 64 && c_in <= 256 && c_in % 64 == 0 && c_out >= 64 && c_out <= 256 && c_out % 64 == 0) ? 1 : 0;
}

extern "C" int pp_conv3x3_wgrad_max_workgroups(void) { return CG_MAX_WG; }

extern "C" long long pp_conv3x3_wgrad_workspace_bytes(int n, int h, int w, int c_in, int c_out) {
    if (n <= 0 || h <= 0 || w <= 0) return PP_ERR_BAD_ARG;
    if (!pp_conv3x3_wgrad_supported(c_in, c_out)) return PP_ERR_UNSUPPORTED;
    const long long rows = (long long)n * h;        // < 2^62
    if (rows > 2147483647ll || rows * w > 2147483647ll) return PP_ERR_TOO_LARGE;
    const long long m = rows * w;
    return 9ll * (c_out / 64) * conv_grid_of(m) * ((long long)HG_KP * c_in + HG_KP) * (long long)sizeof(float);
}

extern "C" int pp_conv3x3_wgrad_f16(const void *dy, const void *x, int n, int h, int w, int c_in, int c_out, float inv_loss_scale,
                                    const float *inv_loss_scale_dev, void *workspace, long long workspace_bytes, float *dw, float *db,
                                    void *stream) {
    if (!dy || !x || !dw || !db || !workspace) return PP_ERR_BAD_ARG;
    if (n <= 0 || h <= 0 || w <= 0) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(dy) % 16 || reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(dw) % 4 ||
        reinterpret_cast<uintptr_t>(db) % 4 || reinterpret_cast<uintptr_t>(workspace) % 4 || reinterpret_cast<uintptr_t>(inv_loss_scale_dev) % 4)
        return PP_ERR_BAD_ARG;
    if (!inv_loss_scale_dev && !(isfinite(inv_loss_scale) && inv_loss_scale > 0.0f)) return PP_ERR_BAD_ARG;
    const long long need = pp_conv3x3_wgrad_workspace_bytes(n, h, w, c_in, c_out);
    if (need < 0) return (int)need;                 // unsupported, then too large
    if (workspace_bytes < need) return PP_ERR_BAD_ARG;
    if (!device_present()) return PP_ERR_NO_DEVICE;

    const long long m = (long long)n * h * w;
    const int n_chunks = (int)n_chunks_of(m), grid = conv_grid_of(m), blocks = 9 * (c_out / 64) * grid;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __half *dyh = static_cast<const __half *>(dy), *xh = static_cast<const __half *>(x);
    float *partial = static_cast<float *>(workspace);
    switch (c_in) {
        case 64: launch_conv<64>(blocks, st, dyh, xh, m, h, w, c_out, n_chunks, grid, partial); break;
        case 128: launch_conv<128>(blocks, st, dyh, xh, m, h, w, c_out, n_chunks, grid, partial); break;
        case 192: launch_conv<192>(blocks, st, dyh, xh, m, h, w, c_out, n_chunks, grid, partial); break;
        default: launch_conv<256>(blocks, st, dyh, xh, m, h, w, c_out, n_chunks, grid, partial); break;
    }
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    hipLaunchKernelGGL(k_conv3x3_wgrad_finish, dim3(c_out * 9 * (c_in / 64) + c_out / 64), dim3(HG_THREADS), 0, st,
                       static_cast<const float *>(partial), grid, c_in, c_out, inv_loss_scale, inv_loss_scale_dev, dw, db);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

extern "C" int pp_conv3x3_dgrad_supported(int c_in, int c_out) { return pp_conv3x3_wgrad_supported(c_in, c_out); }

extern "C" int pp_conv3x3_dgrad_f16(const void *dy, const void *w, const void *y, int n, int h, int wd, int c_in, int c_out, float slope,
                                    void *dx, void *stream) {
    if (!dy || !w || !dx) return PP_ERR_BAD_ARG;
    if (n <= 0 || h <= 0 || wd <= 0) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(dy) % 16 || reinterpret_cast<uintptr_t>(w) % 16 || reinterpret_cast<uintptr_t>(y) % 16 ||
        reinterpret_cast<uintptr_t>(dx) % 16)
        return PP_ERR_BAD_ARG;
    if (y && !(isfinite(slope) && slope > 0.0f)) return PP_ERR_BAD_ARG;
    if (!pp_conv3x3_dgrad_supported(c_in, c_out)) return PP_ERR_UNSUPPORTED;
    const long long rows = (long long)n * h;        // < 2^62
    if (rows > 2147483647ll || rows * wd > 2147483647ll) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;

    const int tiles_x = (wd + CD_T - 1) / CD_T, tiles_y = (h + CD_T - 1) / CD_T;
    const unsigned blocks = (unsigned)((long long)n * tiles_y * tiles_x);      // <= n h w
    hipStream_t st = static_cast<hipStream_t>(stream);
    const __half *dyh = static_cast<const __half *>(dy), *wh = static_cast<const __half *>(w), *yh = static_cast<const __half *>(y);
    __half *dh = static_cast<__half *>(dx);
    switch (c_in) {
        case 64: return launch_conv_dgrad<64>(blocks, st, dyh, wh, yh, h, wd, c_out, tiles_x, tiles_y, slope, dh);
        case 128: return launch_conv_dgrad<128>(blocks, st, dyh, wh, yh, h, wd, c_out, tiles_x, tiles_y, slope, dh);
        case 192: return launch_conv_dgrad<192>(blocks, st, dyh, wh, yh, h, wd, c_out, tiles_x, tiles_y, slope, dh);
        default: return launch_conv_dgrad<256>(blocks, st, dyh, wh, yh, h, wd, c_out, tiles_x, tiles_y, slope, dh);
    }
}
