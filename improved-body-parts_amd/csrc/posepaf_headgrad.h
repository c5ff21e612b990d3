// posepaf_headgrad.h -- the one copy of the reduction GEMM over the pixels that the weight gradients share: the 1 x 1 heads
// (posepaf_headgrad.hip, whose header describes the staging, the transposed LDS reads, the bfloat16 split and the order of the
// additions) and the 3 x 3 convolution (posepaf_convgrad.hip), which runs the same pass once per (tap, 64 output channels) with an
// x load that goes to a pixel's neighbour.  Included by those two files only; everything has internal linkage.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

constexpr int HG_THREADS = 256;
constexpr int HG_P = 64;              // pixels of a chunk
constexpr int HG_MAX_WG = 256;        // one workgroup per CU of an MI355X at the most
constexpr int HG_KP = 64;             // output channels of the tile (rows >= c_out are zero)
constexpr int HG_PAD = 32;            // binary16 elements of padding behind an LDS row (64 bytes)
constexpr int HG_GROW = HG_KP + HG_PAD;

typedef short short4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef __bf16 bf8v __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8v __attribute__((ext_vector_type(8)));
typedef float float16v __attribute__((ext_vector_type(16)));

struct alignas(16) Quad {
    unsigned v[4];
};

struct Frag {
    short4v lo, hi;
};

// pixels row0 .. row0 + 15 (this lane: 8 of them) of the 32 channels from col0 of an LDS image with `stride` elements per row
__device__ __forceinline__ half8v tr_frag(const __half *img, int stride, int row0, int col0, int lane) {
    const int i = lane & 15;
    const __half *p = img + (row0 + 8 * (lane >> 5) + (i >> 2)) * stride + col0 + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
    Frag f;
    f.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v *)p);
    f.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v *)(p + 4 * stride));
    return __builtin_bit_cast(half8v, f);
}

// v = hi + lo exactly, element by element: hi the float32 form cut to bfloat16, lo the rest (<= 3 significant bits)
__device__ __forceinline__ void split_bf16(half8v v, bf8v &hi, bf8v &lo) {
    ushort8v h, l;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float f = (float)v[j];
        const unsigned top = __float_as_uint(f) & 0xffff0000u;
        h[j] = (unsigned short)(top >> 16);
        l[j] = (unsigned short)(__float_as_uint(f - __uint_as_float(top)) >> 16);
    }
    hi = __builtin_bit_cast(bf8v, h), lo = __builtin_bit_cast(bf8v, l);
}

__device__ __forceinline__ unsigned scale2(unsigned x2, unsigned s2) {
    const __half2 x = *reinterpret_cast<const __half2 *>(&x2), s = *reinterpret_cast<const __half2 *>(&s2);
    const __half2 r = __halves2half2(__float2half_rn(__low2float(x) * __low2float(s)), __float2half_rn(__high2float(x) * __high2float(s)));
    return *reinterpret_cast<const unsigned *>(&r);
}

// which row of x pixel p (< m) of g is contracted with: the pixel itself (a 1 x 1 head) ...
struct SamePixel {
    __device__ __forceinline__ long long operator()(long long p) const { return p; }
};

// ... or its neighbour (dr, ds) in the same h x w image, -1 where that lies outside: the row is then zeros and nothing is loaded
struct TapPixel {
    int h, w, dr, ds;
    __device__ __forceinline__ long long operator()(long long p) const {      // p < 2^31
        const unsigned row = (unsigned)p / (unsigned)w;
        const int j = (int)((unsigned)p - row * (unsigned)w), i = (int)(row % (unsigned)h);
        if ((unsigned)(i + dr) >= (unsigned)h || (unsigned)(j + ds) >= (unsigned)w) return -1;
        return p + (long long)dr * w + ds;
    }
};

// The accumulate pass of one head as workgroup `wg` of `grid`: the one copy of the arithmetic, shared by the single entry's kernel,
// the multi-head one and the 3 x 3 convolution's.  GVEC: the rows of g are 16-byte aligned (16-byte loads); else element loads
template <int C_IN, bool GVEC, class XMap>
__device__ __forceinline__ void head_wgrad_accumulate(const __half *__restrict__ g, int ldg, const __half *__restrict__ x,
                                                      const __half *__restrict__ scale, long long m, int hw, int c_out, int n_chunks,
                                                      int grid, int wg, float *__restrict__ partial, const XMap xmap) {
    constexpr int XROW = C_IN + HG_PAD;
    constexpr int VPP = C_IN / 8;                     // 16-byte groups of an x row
    constexpr int NV = HG_P * VPP / HG_THREADS;       // x groups of a thread and chunk
    constexpr bool SAME = HG_THREADS % VPP == 0;      // a thread's groups all sit at one channel offset
    constexpr int NS = SAME ? 1 : NV;
    constexpr int NB = C_IN / 64;                     // 32-column tiles of a wave

    __shared__ alignas(16) __half s_x[HG_P * XROW];
    __shared__ alignas(16) __half s_g[HG_P * HG_GROW];
    __shared__ float s_db[HG_THREADS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    Quad xr[NV], sr[NS], gq[GVEC ? 2 : 1];
    unsigned short ge[GVEC ? 1 : 16];

    auto load_chunk = [&](int chunk) {
        const long long p0 = (long long)chunk * HG_P;
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const int v = tid + HG_THREADS * i, pix = v / VPP, cv = v - pix * VPP;
            xr[i] = Quad{{0u, 0u, 0u, 0u}};
            if (p0 + pix < m) {
                const long long src = xmap(p0 + pix);
                if (src >= 0) xr[i] = *reinterpret_cast<const Quad *>(x + (size_t)src * C_IN + cv * 8);
            }
        }
        if (scale) {
            const __half *srow = scale + (size_t)(p0 / hw) * C_IN;     // hw % 64 == 0: a chunk lies in one image
#pragma unroll
            for (int i = 0; i < NS; i++) {
                const int v = tid + HG_THREADS * i;
                sr[i] = *reinterpret_cast<const Quad *>(srow + (v % VPP) * 8);
            }
        }
        if (GVEC) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int v = tid + HG_THREADS * i, pix = v >> 3, c0 = (v & 7) * 8;
                Quad q = Quad{{0u, 0u, 0u, 0u}};
                if (p0 + pix < m && c0 < c_out) {
                    q = *reinterpret_cast<const Quad *>(g + (size_t)(p0 + pix) * ldg + c0);
#pragma unroll
                    for (int j = 0; j < 4; j++) {     // padding channels of a straddling group: replaced, never computed with
                        if (c0 + 2 * j >= c_out) q.v[j] = 0u;
                        else if (c0 + 2 * j + 1 >= c_out) q.v[j] &= 0xffffu;
                    }
                }
                gq[i] = q;
            }
        } else {
            const unsigned short *gs = reinterpret_cast<const unsigned short *>(g);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int e = tid + HG_THREADS * i, pix = e >> 6, c = e & 63;
                ge[i] = (p0 + pix < m && c < c_out) ? gs[(size_t)(p0 + pix) * ldg + c] : (unsigned short)0;
            }
        }
    };

    auto stage_chunk = [&]() {
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const int v = tid + HG_THREADS * i, pix = v / VPP, cv = v - pix * VPP;
            Quad q = xr[i];
            if (scale) {
                const Quad s = sr[SAME ? 0 : i];
#pragma unroll
                for (int j = 0; j < 4; j++) q.v[j] = scale2(q.v[j], s.v[j]);
            }
            *reinterpret_cast<Quad *>(s_x + pix * XROW + cv * 8) = q;
        }
        if (GVEC) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int v = tid + HG_THREADS * i;
                *reinterpret_cast<Quad *>(s_g + (v >> 3) * HG_GROW + (v & 7) * 8) = gq[i];
            }
        } else {
            unsigned short *sg = reinterpret_cast<unsigned short *>(s_g);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int e = tid + HG_THREADS * i;
                sg[(e >> 6) * HG_GROW + (e & 63)] = ge[i];
            }
        }
    };

    float16v acc[NB];
#pragma unroll
    for (int j = 0; j < NB; j++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[j][r] = 0.0f;
    float dbacc = 0.0f;
    const int row_tile = wave & 1, col_tile0 = wave >> 1;

    load_chunk(wg);                                   // grid <= n_chunks: every workgroup has a first chunk
    for (int chunk = wg; chunk < n_chunks; chunk += grid) {
        __syncthreads();                              // the previous chunk's reads of the LDS images are done
        stage_chunk();
        __syncthreads();
        if (chunk + grid < n_chunks) load_chunk(chunk + grid);
#pragma unroll
        for (int ks = 0; ks < HG_P / 16; ks++) {
            bf8v a_hi, a_lo;
            split_bf16(tr_frag(s_g, HG_GROW, 16 * ks, 32 * row_tile, lane), a_hi, a_lo);
#pragma unroll
            for (int j = 0; j < NB; j++) {
                bf8v b_hi, b_lo;
                split_bf16(tr_frag(s_x, XROW, 16 * ks, 32 * (col_tile0 + 2 * j), lane), b_hi, b_lo);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, b_lo, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, b_lo, acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; i++) dbacc += __half2float(s_g[(16 * wave + i) * HG_GROW + lane]);
    }

    float *out = partial + (size_t)wg * ((size_t)c_out * C_IN + c_out);
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const int col = 32 * (col_tile0 + 2 * j) + (lane & 31);
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = 32 * row_tile + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (row < c_out) out[(size_t)row * C_IN + col] = acc[j][r];
        }
    }
    s_db[tid] = dbacc;
    __syncthreads();
    if (tid < c_out) out[(size_t)c_out * C_IN + tid] = ((s_db[tid] + s_db[64 + tid]) + s_db[128 + tid]) + s_db[192 + tid];
}

inline int device_present() {
    static int have = -1;
    if (have < 0) {
        int n = 0;
        have = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    }
    return have;
}

inline long long n_chunks_of(long long m) { return (m + HG_P - 1) / HG_P; }

}  // namespace
