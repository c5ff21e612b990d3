// posepaf_headopt.hip -- the optimiser step of the 1 x 1 heads' float32 masters in one chain of two launches (include/posepaf.h):
//   k_head_update_flags: workgroup b ORs "not finite" over its share of the n gradients and stores ONE flag word with a plain store,
//     on every launch (nothing is zeroed beforehand and nothing is added atomically: DESIGN section 3, "The status words").
//   k_head_update: every workgroup ORs the flag words.  All finite: torch.optim.SGD's update, each operation rounded where torch's
//     kernels on this build round it (found by comparing with torch.optim.SGD on the MI355X):
//       g'   = fma(wd, p, g)          _foreach_add(grads, params, alpha = wd) contracts;   wd == 0: g' = g, as torch skips the operation
//       buf' = fl(mu * buf) + g'      _foreach_mul_(bufs, mu), then _foreach_add_(bufs, grads): two kernels, two roundings
//       p'   = fma(-lr, buf', p)      _foreach_add_(params, bufs, alpha = -lr) contracts;  mu == 0: buf' = g', no buffer read or written
//     written with __fmaf_rn / __fmul_rn / __fadd_rn, so the file does not depend on the compiler's contraction flag; then every
//     master inside a head's range is rounded to binary16 (nearest even) into its two destinations.  One not finite: nothing but the
//     state block is written.  Thread 0 of workgroup 0 then runs the loss-scale state machine (apex's dynamic scaler).
// pp_layer_update_f32 is the same chain with a table of up to PP_LAYER_UPDATE_MAX_SEGMENTS single segments in place of the heads'
// descriptors: k_head_update is a template over where its segments come from, so the arithmetic exists once.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "posepaf_internal.h"

namespace {

constexpr int HO_THREADS = 256;
constexpr int HO_MAX_WG = 256;                    // workgroups of either launch; also the flag words
constexpr int HO_PER_WG = 4 * HO_THREADS;         // gradients a workgroup of the first launch tests per pass
constexpr int HO_SEGS = 2 * PP_HEAD_WGRAD_MULTI_MAX;

int grid_of(long long n) {
    const long long g = (n + HO_PER_WG - 1) / HO_PER_WG;
    return (int)(g < HO_MAX_WG ? g : HO_MAX_WG);
}

__global__ __launch_bounds__(HO_THREADS) void k_head_update_flags(const float *__restrict__ grads, int n, unsigned *__restrict__ flags) {
    int bad = 0;
    for (int i = (int)blockIdx.x * HO_THREADS + (int)threadIdx.x; i < n; i += (int)gridDim.x * HO_THREADS)
        bad |= (__float_as_uint(grads[i]) & 0x7f800000u) == 0x7f800000u;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) flags[blockIdx.x] = bad ? 1u : 0u;
}

// where k_head_update's segments come from: a segment is a range [start, start + len) of the flat tensors and its two binary16
// destinations.  A head's descriptor is two segments (weight, bias) ...
struct HeadTable {
    const pp_head_update_desc *__restrict__ table;
    int n_heads;
    __device__ __forceinline__ int segments() const { return 2 * n_heads; }
    __device__ __forceinline__ void load(int tid, long long *start, long long *len, __half *(*dst)[2]) const {
        if (tid < n_heads) {
            const pp_head_update_desc d = table[tid];
            start[2 * tid] = d.w_off, len[2 * tid] = d.w_len;
            dst[2 * tid][0] = static_cast<__half *>(d.weight), dst[2 * tid][1] = static_cast<__half *>(d.wpad);
            start[2 * tid + 1] = d.b_off, len[2 * tid + 1] = d.b_len;
            dst[2 * tid + 1][0] = static_cast<__half *>(d.bias), dst[2 * tid + 1][1] = static_cast<__half *>(d.bpad);
        }
    }
};

// ... and pp_layer_update_f32's table names them one by one
struct SegmentTable {
    const pp_update_segment *__restrict__ table;
    int n_segments;
    __device__ __forceinline__ int segments() const { return n_segments; }
    __device__ __forceinline__ void load(int tid, long long *start, long long *len, __half *(*dst)[2]) const {
        if (tid < n_segments) {                       // n_segments <= HO_THREADS
            const pp_update_segment d = table[tid];
            start[tid] = d.off, len[tid] = d.len;
            dst[tid][0] = static_cast<__half *>(d.dst), dst[tid][1] = static_cast<__half *>(d.dst2);
        }
    }
};

static_assert(PP_LAYER_UPDATE_MAX_SEGMENTS <= HO_THREADS && PP_HEAD_WGRAD_MULTI_MAX <= HO_THREADS, "one thread loads one table entry");

// the one copy of the update's arithmetic: both entries launch it, with their table and its capacity
template <int MAX_SEGS, class Table>
__global__ __launch_bounds__(HO_THREADS) void k_head_update(float *__restrict__ masters, const float *__restrict__ grads,
                                                             float *__restrict__ momentum, int n, const Table table,
                                                             const float *__restrict__ hyper, pp_head_update_state *state,
                                                             const unsigned *__restrict__ flags, int n_flags) {
    __shared__ long long s_start[MAX_SEGS], s_len[MAX_SEGS];
    __shared__ __half *s_dst[MAX_SEGS][2];
    const int tid = (int)threadIdx.x;
    const int skip = __syncthreads_or(tid < n_flags ? (int)flags[tid] : 0);      // n_flags <= HO_THREADS

    if (!skip) {
        table.load(tid, s_start, s_len, s_dst);
        __syncthreads();
        const float lr = hyper[0], mu = hyper[1], wd = hyper[2];
        const int n_seg = table.segments();
        for (int i = (int)blockIdx.x * HO_THREADS + tid; i < n; i += (int)gridDim.x * HO_THREADS) {
            const float p = masters[i], g = grads[i];
            const float g1 = wd != 0.0f ? __fmaf_rn(wd, p, g) : g;
            float b1 = g1;
            if (mu != 0.0f) {
                b1 = __fadd_rn(__fmul_rn(mu, momentum[i]), g1);
                momentum[i] = b1;
            }
            const float p1 = __fmaf_rn(-lr, b1, p);
            masters[i] = p1;
            int lo = 0, hi = n_seg;                    // the last range that starts at or before i (ranges ascend)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_start[mid] <= i) lo = mid + 1;
                else hi = mid;
            }
            const int s = lo - 1;
            if (s >= 0 && i - s_start[s] < s_len[s]) {
                const __half h = __float2half_rn(p1);
                const long long j = i - s_start[s];
                s_dst[s][0][j] = h, s_dst[s][1][j] = h;
            }
        }
    }

    if (blockIdx.x == 0 && tid == 0) {
        pp_head_update_state st = *state;
        if (skip) st.skipped += 1;
        if (st.growth_interval > 0) {
            if (skip) {
                const float half = __fmul_rn(st.scale, 0.5f);
                st.scale = half > st.min_scale ? half : st.min_scale;
                st.good_steps = 0;
            } else if (++st.good_steps >= st.growth_interval) {
                const float twice = __fmul_rn(st.scale, 2.0f);
                st.scale = twice < st.max_scale ? twice : st.max_scale;
                st.good_steps = 0;
            }
            st.inv_scale = __fdiv_rn(1.0f, st.scale);
        }
        *state = st;
    }
}

// the chain of two launches both entries share
template <int MAX_SEGS, class Table>
int launch_update(float *masters, const float *grads, float *momentum, long n, const Table table, const float *hyper,
                  pp_head_update_state *state, void *workspace, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int grid = grid_of(n);
    unsigned *flags = static_cast<unsigned *>(workspace);
    hipLaunchKernelGGL(k_head_update_flags, dim3(grid), dim3(HO_THREADS), 0, st, grads, (int)n, flags);
    if (hipGetLastError() != hipSuccess) return PP_ERR_HIP;
    hipLaunchKernelGGL((k_head_update<MAX_SEGS, Table>), dim3(grid), dim3(HO_THREADS), 0, st, masters, grads, momentum, (int)n, table, hyper,
                       state, static_cast<const unsigned *>(flags), grid);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

int device_present() {
    static int have = -1;
    if (have < 0) {
        int n = 0;
        have = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
    }
    return have;
}

}  // namespace

extern "C" long long pp_head_update_workspace_bytes(long n) {
    if (n <= 0) return PP_ERR_BAD_ARG;
    if ((long long)n > 2147483647ll) return PP_ERR_TOO_LARGE;
    return (long long)grid_of(n) * (long long)sizeof(unsigned);
}

extern "C" int pp_head_update_f32(float *masters, const float *grads, float *momentum, long n, const pp_head_update_desc *table, int n_heads,
                                  const float *hyper, pp_head_update_state *state, void *workspace, void *stream) {
    if (!masters || !grads || !momentum || !table || !hyper || !state || !workspace) return PP_ERR_BAD_ARG;
    if (n <= 0 || n_heads < 0) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(masters) % 4 || reinterpret_cast<uintptr_t>(grads) % 4 || reinterpret_cast<uintptr_t>(momentum) % 4 ||
        reinterpret_cast<uintptr_t>(hyper) % 4 || reinterpret_cast<uintptr_t>(workspace) % 4 || reinterpret_cast<uintptr_t>(table) % 8 ||
        reinterpret_cast<uintptr_t>(state) % 8)
        return PP_ERR_BAD_ARG;
    if (n_heads > PP_HEAD_WGRAD_MULTI_MAX) return PP_ERR_UNSUPPORTED;
    if ((long long)n > 2147483647ll) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;
    return launch_update<HO_SEGS>(masters, grads, momentum, n, HeadTable{table, n_heads}, hyper, state, workspace, stream);
}

extern "C" int pp_layer_update_max_segments(void) { return PP_LAYER_UPDATE_MAX_SEGMENTS; }

extern "C" int pp_layer_update_f32(float *masters, const float *grads, float *momentum, long n, const pp_update_segment *segments,
                                   int n_segments, const float *hyper, pp_head_update_state *state, void *workspace, void *stream) {
    if (!masters || !grads || !momentum || !segments || !hyper || !state || !workspace) return PP_ERR_BAD_ARG;
    if (n <= 0 || n_segments < 0) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(masters) % 4 || reinterpret_cast<uintptr_t>(grads) % 4 || reinterpret_cast<uintptr_t>(momentum) % 4 ||
        reinterpret_cast<uintptr_t>(hyper) % 4 || reinterpret_cast<uintptr_t>(workspace) % 4 || reinterpret_cast<uintptr_t>(segments) % 8 ||
        reinterpret_cast<uintptr_t>(state) % 8)
        return PP_ERR_BAD_ARG;
    if (n_segments > PP_LAYER_UPDATE_MAX_SEGMENTS) return PP_ERR_UNSUPPORTED;
    if ((long long)n > 2147483647ll) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;
    return launch_update<PP_LAYER_UPDATE_MAX_SEGMENTS>(masters, grads, momentum, n, SegmentTable{segments, n_segments}, hyper, state, workspace,
                                                       stream);
}
