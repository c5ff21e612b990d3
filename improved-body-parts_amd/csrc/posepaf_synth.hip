// posepaf_synth.hip -- ground-truth-style scenes rendered where the post-processing reads them: joint lists in, the network-output
// layout (B, n_samples, 50, h, w) out, one launch for the whole batch.  The recipe is the reference's training-target recipe
// (py_cocodata_server/py_data_heatmapper.py:105-257, restated on the host in posepaf/synth.py render_maps / mirror_sample):
//   keypoint channel 30 + k   max over people of expf(-(gx - x)^2 / 162f) * expf(-(gy - y)^2 / 162f), float32, gx = 4 i + 1.5,
//                             inside the window round(x / 4) - 7 .. + 7 cells (:117-164)
//   limb channel l            inside the end points' bounding box grown by 4 px, in float64 (:326-357):
//                                 d = |dx (y1 - Y) - (x1 - X) dy| / (norm + 1e-6),  g = exp(-d^2 / 98),  g <= 0.015 -> 0.01
//                             summed in person order as float32 += float64 (acc = (float)((double)acc + g), what NumPy's in-place
//                             add does), divided by the number of contributions where there is one (:239-244)
//   clip to [0, 1]; channel 48 zero (no segmentation mask here); channel 49 zero, or with PP_SCENE_REVERSE_KP the max over the 18
//   keypoint channels (:86); sample 1 = the mirrored scene with the left / right channels exchanged (synth.mirror_sample).
// GATHER: a workgroup takes one 64 x 32 tile of one image and a residue class of the channels; a thread owns 8 consecutive x of
// one row and walks the people of its image IN INDEX ORDER, so there are no atomics, the result is deterministic and the float32
// accumulation order is the reference's.  The image's joints and the per-(person, channel) windows, clipped to the tile, are
// staged in LDS once per workgroup; people none of whose windows reach the tile are dropped from the walk.  Every output word of
// the batch is stored plainly on every launch (no memset).  Window arithmetic is float64 on the float32 joint values; round is
// round-half-to-even (rint), as Python's.  Compiled with -ffp-contract=off: products and sums round separately.
// Noise (optional): out = clip(v) + sigma * N(0, 1), no second clip; N from Philox4x32-10 keyed by the seed with the counter
// (pixel group, channel | sample << 8, scene id low, scene id high) and Box-Muller in float32 -- no state, nothing that depends on
// the launch geometry, the batch composition or the slot.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "posepaf_internal.h"

namespace {

constexpr int SC_TW = 64, SC_TH = 32;         // tile: 8 threads x 8 pixels wide (one 128-byte fp16 line), 32 rows
constexpr int SC_THREADS = 256;
constexpr int SC_PX = 8;
#ifndef SC_MIN_WAVES
#define SC_MIN_WAVES 4
#endif
constexpr int SC_NWIN = PP_NUM_LIMB + PP_NUM_PART;   // windows per person: 30 limbs, then 18 keypoints

// the library's limb and flip tables: the lists of posepaf_internal.h that posepaf_kernels.hip's arrays are made from (this
// translation unit needs device arrays of its own: no relocatable device code)
__device__ const int8_t d_limb_from[PP_NUM_LIMB] = PP_LIMB_FROM_LIST;
__device__ const int8_t d_limb_to[PP_NUM_LIMB] = PP_LIMB_TO_LIST;
__device__ const int8_t d_flip_heat_ord[PP_NUM_HEAT] = PP_FLIP_HEAT_ORD_LIST;
__device__ const int8_t d_flip_paf_ord[PP_NUM_LIMB] = PP_FLIP_PAF_ORD_LIST;

// int(round(v)) of Python for a float64: ties to even; saturated far outside any map (a NaN lands on the lower bound)
__device__ __forceinline__ int round_cell(double v) { return (int)rint(fmin(fmax(v, -1.0e9), 1.0e9)); }

// [lo, hi) x [ylo, yhi) in map cells -> the part inside the tile, tile-local, packed x0 | x1 << 7 | y0 << 14 | y1 << 20; 0 = none
__device__ __forceinline__ unsigned pack_window(int x0, int x1, int y0, int y1, int tx0, int ty0, int tx1, int ty1) {
    x0 = max(x0, tx0) - tx0, x1 = min(x1, tx1) - tx0;
    y0 = max(y0, ty0) - ty0, y1 = min(y1, ty1) - ty0;
    if (x1 <= x0 || y1 <= y0) return 0u;
    return (unsigned)x0 | ((unsigned)x1 << 7) | ((unsigned)y0 << 14) | ((unsigned)y1 << 20);
}

// ---- Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1, c[3] = (unsigned)p0, c[0] = n0, c[2] = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the four normals of pixel group `grp` (pixels 4 grp .. 4 grp + 3 of the plane, row-major) of (scene, sample, channel)
__device__ __forceinline__ void normals4(float z[4], unsigned long long seed, long long scene, int sample, int ch, unsigned grp) {
    unsigned c[4] = {grp, (unsigned)ch | ((unsigned)sample << 8), (unsigned)(unsigned long long)scene,
                     (unsigned)((unsigned long long)scene >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
    for (int i = 0; i < 2; i++) {
        // u1 in (0, 1], u2 in [0, 1): 2^-32 steps
        const float u1 = fminf((float)c[2 * i] * 2.3283064365386963e-10f + 1.1641532182693481e-10f, 1.0f);
        const float u2 = (float)c[2 * i + 1] * 2.3283064365386963e-10f;
        // the hardware log2 / sin / cos: the noise is defined by this code, not by a libm, and only its distribution matters
        const float r = sqrtf(-2.0f * __logf(u1));
        const float a = 6.2831853071795865f * u2;
        z[2 * i] = r * __cosf(a), z[2 * i + 1] = r * __sinf(a);
    }
}

// noise of the SC_PX pixels lin0 .. lin0 + 7 of a plane (lin = y * w + x; entries of pixels outside the map are never stored)
__device__ __forceinline__ void noise8(float n[SC_PX], float sigma, unsigned long long seed, long long scene, int sample, int ch,
                                       long long lin0) {
    if ((lin0 & 3) == 0) {                                   // every run of a map whose width is a multiple of 4: two whole groups
        normals4(n, seed, scene, sample, ch, (unsigned)(lin0 >> 2));
        normals4(n + 4, seed, scene, sample, ch, (unsigned)(lin0 >> 2) + 1u);
#pragma unroll
        for (int j = 0; j < SC_PX; j++) n[j] *= sigma;
        return;
    }
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    long long have = (lin0 >> 2) - 1;
#pragma unroll 1
    for (int j = 0; j < SC_PX; j++) {                        // one copy of the generator's code; n[j] through selects
        const long long lin = lin0 + j, grp = lin >> 2;
        if (grp != have) normals4(z, seed, scene, sample, ch, (unsigned)grp), have = grp;
        const int lane = (int)(lin & 3);
        const float val = sigma * (lane == 0 ? z[0] : lane == 1 ? z[1] : lane == 2 ? z[2] : z[3]);
#pragma unroll
        for (int k = 0; k < SC_PX; k++)
            if (k == j) n[k] = val;
    }
}

template <typename T>
__device__ __forceinline__ T to_out(float v);
template <>
__device__ __forceinline__ float to_out<float>(float v) { return v; }
template <>
__device__ __forceinline__ __half to_out<__half>(float v) { return __float2half_rn(v); }

template <typename T>
struct alignas(sizeof(T) * SC_PX) Vec8 {
    T v[SC_PX];
};

// v[j] -> row[x + j] for the npx pixels of the thread inside the map; one 16-byte (fp16) / two 16-byte (fp32) stores when VEC
template <typename T>
__device__ __forceinline__ void store_run(T *row, int x, const float v[SC_PX], int npx, bool vec) {
    if (vec && npx == SC_PX) {
        Vec8<T> o;
#pragma unroll
        for (int j = 0; j < SC_PX; j++) o.v[j] = to_out<T>(v[j]);
        *reinterpret_cast<Vec8<T> *>(row + x) = o;
    } else {
        for (int j = 0; j < npx; j++) row[x + j] = to_out<T>(v[j]);
    }
}

// one keypoint channel's contribution of the listed people to the thread's pixels: acc = max(acc, ey * ex)
__device__ __forceinline__ void gather_keypoint(float acc[SC_PX], int part, const float *s_joints, const unsigned *s_win,
                                                const unsigned char *s_list, int nsurv, int lx, int ly, float gx0, float gy) {
    for (int s = 0; s < nsurv; s++) {
        const int p = s_list[s];
        const unsigned wv = s_win[p * SC_NWIN + PP_NUM_LIMB + part];
        if (wv == 0u) continue;
        const int x0 = wv & 127, x1 = (wv >> 7) & 127, y0 = (wv >> 14) & 63, y1 = (wv >> 20) & 63;
        if (ly < y0 || ly >= y1 || lx + SC_PX <= x0 || lx >= x1) continue;
        const float jx = s_joints[(p * PP_NUM_PART + part) * 3], jy = s_joints[(p * PP_NUM_PART + part) * 3 + 1];
        const float ty = gy - jy;
        const float ey = expf(-(ty * ty) / 162.0f);
#pragma unroll
        for (int j = 0; j < SC_PX; j++) {
            if (lx + j < x0 || lx + j >= x1) continue;
            const float tx = (gx0 + 4.0f * (float)j) - jx;       // 4 i + 1.5 is exact in float32 for every map this library takes
            const float ex = expf(-(tx * tx) / 162.0f);
            acc[j] = fmaxf(acc[j], ey * ex);
        }
    }
}

struct LdsLayout {
    unsigned win, list, keep, nsurv, bytes;
};
__host__ __device__ inline LdsLayout lds_layout(int max_people) {
    LdsLayout l;
    l.win = ((unsigned)max_people * PP_NUM_PART * 3 * 4 + 15u) & ~15u;
    l.list = l.win + (unsigned)max_people * SC_NWIN * 4;          // 192 bytes per person
    l.keep = l.list + (((unsigned)max_people + 15u) & ~15u);
    l.nsurv = l.keep + (((unsigned)max_people + 15u) & ~15u);
    l.bytes = l.nsurv + 16u;
    return l;
}

template <typename T>
__global__ __launch_bounds__(SC_THREADS, SC_MIN_WAVES) void k_render_scenes(const float *__restrict__ joints, const int *__restrict__ n_people,
                                                              const long long *__restrict__ scene_id, int batch, int max_people,
                                                              int h, int w, int n_samples, int flags, float sigma,
                                                              unsigned long long seed, T *__restrict__ out, int tiles_x, int vec) {
    // all LDS in the dynamic region, every carve on a 16-byte boundary (lds_layout below)
    extern __shared__ __align__(16) unsigned char s_raw[];
    const LdsLayout lay = lds_layout(max_people);
    float *s_joints = reinterpret_cast<float *>(s_raw);                       // [max_people][18][3]
    unsigned *s_win = reinterpret_cast<unsigned *>(s_raw + lay.win);          // [max_people][48]
    unsigned char *s_list = s_raw + lay.list;                                 // [max_people]
    unsigned char *s_keep = s_raw + lay.keep;                                 // [max_people]: 1 = some window reaches the tile
    int *s_nsurv = reinterpret_cast<int *>(s_raw + lay.nsurv);

    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = (int)(blockIdx.x % tiles_x) * SC_TW, ty0 = (int)(blockIdx.x / tiles_x) * SC_TH;
    const int tx1 = min(tx0 + SC_TW, w), ty1 = min(ty0 + SC_TH, h);   // exclusive
    const int P = min(max(n_people[b], 0), max_people);

    // ---- the image's joints, then every (person, channel) window clipped to this tile
    const float *jb = joints + (size_t)b * max_people * PP_NUM_PART * 3;
    for (int i = tid; i < P * PP_NUM_PART * 3; i += SC_THREADS) s_joints[i] = jb[i];
    if (tid < P) s_keep[tid] = 0;
    __syncthreads();
    for (int i = tid; i < P * SC_NWIN; i += SC_THREADS) {
        const int p = i / SC_NWIN, c = i - p * SC_NWIN;
        const float *jp = s_joints + p * PP_NUM_PART * 3;
        unsigned wv = 0u;
        if (c >= PP_NUM_LIMB) {
            const float *j = jp + (c - PP_NUM_LIMB) * 3;
            if (j[2] < 2.0f) {
                const int cx = round_cell((double)j[0] / 4.0), cy = round_cell((double)j[1] / 4.0);
                if (cx + 8 >= 0 && cy + 8 >= 0) wv = pack_window(max(cx - 7, 0), cx + 8, max(cy - 7, 0), cy + 8, tx0, ty0, tx1, ty1);
            }
        } else {
            const float *ja = jp + d_limb_from[c] * 3, *jc = jp + d_limb_to[c] * 3;
            if (ja[2] < 2.0f && jc[2] < 2.0f) {
                const double x1 = ja[0], y1 = ja[1], x2 = jc[0], y2 = jc[1];
                const double dx = x2 - x1, dy = y2 - y1;
                const double dx2 = dx * dx, dy2 = dy * dy;
                if (dx2 + dy2 != 0.0) {   // a NaN coordinate passes here and yields NaN pixels inside a clipped window, never an address
                    const int sx0 = round_cell((fmin(x1, x2) - 4.0) / 4.0), sy0 = round_cell((fmin(y1, y2) - 4.0) / 4.0);
                    const int sx1 = round_cell((fmax(x1, x2) + 4.0) / 4.0), sy1 = round_cell((fmax(y1, y2) + 4.0) / 4.0);
                    if (sx1 >= 0 && sy1 >= 0) wv = pack_window(max(sx0, 0), sx1 + 1, max(sy0, 0), sy1 + 1, tx0, ty0, tx1, ty1);
                }
            }
        }
        s_win[i] = wv;
        if (wv != 0u) s_keep[p] = 1;      // several threads may store the same 1: no read-modify-write, no conflict-heavy scan later
    }
    __syncthreads();
    // ---- people with a window in the tile, in index order (max_people <= 64: one wave holds them all)
    if (tid < 64) {
        const bool keep = tid < P && s_keep[tid] != 0;
        const unsigned long long m = __ballot(keep);
        if (keep) s_list[__popcll(m & ((1ull << tid) - 1ull))] = (unsigned char)tid;
        if (tid == 0) *s_nsurv = __popcll(m);
    }
    __syncthreads();
    const int nsurv = *s_nsurv;

    // ---- the thread's pixels
    const int lx = (tid & 7) * SC_PX, ly = tid >> 3;
    const int x = tx0 + lx, y = ty0 + ly;
    const int npx = y < h ? min(max(w - x, 0), SC_PX) : 0;
    if (npx == 0) return;                                       // no barrier below this line
    const float gx0 = 4.0f * (float)x + 1.5f, gy = 4.0f * (float)y + 1.5f;
    const double gyd = 4.0 * (double)y + 1.5;
    const size_t plane = (size_t)h * w;
    const long long sid = scene_id ? scene_id[b] : (long long)b;
    const bool noisy = sigma > 0.0f;

    for (int c = blockIdx.y; c < PP_NUM_CH; c += gridDim.y) {
        float v[SC_PX];
#pragma unroll
        for (int j = 0; j < SC_PX; j++) v[j] = 0.0f;
        if (c < PP_NUM_LIMB) {
            int cnt[SC_PX];
#pragma unroll
            for (int j = 0; j < SC_PX; j++) cnt[j] = 0;
            const int a = d_limb_from[c], e = d_limb_to[c];
            for (int s = 0; s < nsurv; s++) {
                const int p = s_list[s];
                const unsigned wv = s_win[p * SC_NWIN + c];
                if (wv == 0u) continue;
                const int x0 = wv & 127, x1 = (wv >> 7) & 127, y0 = (wv >> 14) & 63, y1 = (wv >> 20) & 63;
                if (ly < y0 || ly >= y1 || lx + SC_PX <= x0 || lx >= x1) continue;
                const float *ja = s_joints + (p * PP_NUM_PART + a) * 3, *je = s_joints + (p * PP_NUM_PART + e) * 3;
                const double ax = ja[0], ay = ja[1];
                const double dx = (double)je[0] - ax, dy = (double)je[1] - ay;
                const double dx2 = dx * dx, dy2 = dy * dy;
                const double den = sqrt(dx2 + dy2) + 1e-6;
                const double ty = dx * (ay - gyd);
#pragma unroll 1
                for (int j = 0; j < SC_PX; j++) {                  // one copy of the float64 code; v[j] through selects
                    if (lx + j < x0 || lx + j >= x1) continue;
                    const double gxd = 4.0 * (double)(x + j) + 1.5;
                    const double tx = (ax - gxd) * dy;
                    const double d = fabs(ty - tx) / den;
                    const double d2 = d * d;
                    // exp(-412 / 98) = 0.01493 < 0.015: beyond it the floor applies whatever exp's last bits are (most of a
                    // slanted limb's box lies there), so exp is evaluated near the limb only
                    double g = 0.01;
                    if (!(d2 >= 412.0)) {
                        g = exp(-d2 / 98.0);
                        if (g <= 0.015) g = 0.01;
                    }
#pragma unroll
                    for (int k = 0; k < SC_PX; k++)
                        if (k == j) v[k] = (float)((double)v[k] + g), cnt[k]++;
                }
            }
#pragma unroll
            for (int j = 0; j < SC_PX; j++)
                if (cnt[j] > 0) v[j] = v[j] / (float)cnt[j];
        } else if (c < PP_NUM_LIMB + PP_NUM_PART) {
            gather_keypoint(v, c - PP_NUM_LIMB, s_joints, s_win, s_list, nsurv, lx, ly, gx0, gy);
        } else if (c == PP_NUM_CH - 1 && (flags & PP_SCENE_REVERSE_KP)) {
            for (int part = 0; part < PP_NUM_PART; part++) gather_keypoint(v, part, s_joints, s_win, s_list, nsurv, lx, ly, gx0, gy);
        }
#pragma unroll
        for (int j = 0; j < SC_PX; j++) v[j] = fminf(fmaxf(v[j], 0.0f), 1.0f);

        // sample 0
        float o[SC_PX];
        if (noisy) {
            noise8(o, sigma, seed, sid, 0, c, (long long)y * w + x);
#pragma unroll
            for (int j = 0; j < SC_PX; j++) o[j] = v[j] + o[j];
        } else {
#pragma unroll
            for (int j = 0; j < SC_PX; j++) o[j] = v[j];
        }
        T *row0 = out + ((size_t)b * n_samples * PP_NUM_CH + c) * plane + (size_t)y * w;
        store_run<T>(row0, x, o, npx, vec != 0);

        // sample 1: out1[cf][y][w - 1 - (x + j)] = out0[c][y][x + j], cf = the mirrored channel (the orders are involutions)
        if (n_samples == 2) {
            const int cf = c < PP_NUM_LIMB ? d_flip_paf_ord[c] : PP_NUM_LIMB + d_flip_heat_ord[c - PP_NUM_LIMB];
            const int xm = w - SC_PX - x;                        // x of the run's first pixel; < 0 only when npx < 8
            float n1[SC_PX];
#pragma unroll
            for (int j = 0; j < SC_PX; j++) n1[j] = 0.0f;
            if (noisy) noise8(n1, sigma, seed, sid, 1, cf, (long long)y * w + xm);
            float m[SC_PX];
#pragma unroll
            for (int j = 0; j < SC_PX; j++) m[j] = v[SC_PX - 1 - j] + n1[j];
            T *row1 = out + (((size_t)b * n_samples + 1) * PP_NUM_CH + cf) * plane + (size_t)y * w;
            if (npx == SC_PX) {
                store_run<T>(row1, xm, m, SC_PX, vec != 0);
            } else {
                for (int j = SC_PX - npx; j < SC_PX; j++) row1[xm + j] = to_out<T>(m[j]);   // xm + j = w - 1 - (x + 7 - j) >= 0
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

}  // namespace

extern "C" int pp_render_scenes(const float *joints_dev, const int *n_people_dev, const long long *scene_id_dev, int batch,
                                int max_people, int h, int w, int n_samples, int dtype, int flags, float noise_sigma,
                                unsigned long long seed, void *out_dev, void *stream) {
    if (!joints_dev || !n_people_dev || !out_dev || batch <= 0 || max_people <= 0 || h <= 0 || w <= 0) return PP_ERR_BAD_ARG;
    if ((n_samples != 1 && n_samples != 2) || (dtype != PP_F16 && dtype != PP_F32)) return PP_ERR_BAD_ARG;
    if (!(noise_sigma >= 0.0f)) return PP_ERR_BAD_ARG;
    if (max_people > PP_SCENE_MAX_PEOPLE) return PP_ERR_UNSUPPORTED;
    const long tiles_x = ((long)w + SC_TW - 1) / SC_TW, tiles_y = ((long)h + SC_TH - 1) / SC_TH;
    // pixel coordinates 4 i + 1.5 stay exact in float32 and a plane's pixel groups fit the 32-bit counter word
    // and a launch holds fewer than 2^32 threads in x: fewer than 2^24 tiles of 256 threads (a map of about 3.4e10 pixels)
    if (h > 1000000 || w > 1000000 || tiles_x * tiles_y >= (1L << 24) || (long)h * w > (1L << 33)) return PP_ERR_TOO_LARGE;
    if (batch > 65535) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;
    // channel classes per tile: enough workgroups to fill the chip at small batches, one LDS staging per tile at large ones
    const long tiles = tiles_x * tiles_y * batch;
    const int splits[5] = {2, 5, 10, 25, 50};
    int split = 1;
    for (int i = 0; i < 5; i++)
        if (tiles * split < 4096) split = splits[i];
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)split, (unsigned)batch), block(SC_THREADS);
    const size_t lds = lds_layout(max_people).bytes;               // 26.3 KB at PP_SCENE_MAX_PEOPLE
    const size_t esz = dtype == PP_F16 ? 2 : 4;
    // 8-pixel runs as whole aligned vectors: every row start and the base on a run boundary
    const int vec = (w % SC_PX == 0) && (reinterpret_cast<uintptr_t>(out_dev) % (esz * SC_PX) == 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == PP_F16)
        hipLaunchKernelGGL(k_render_scenes<__half>, grid, block, lds, st, joints_dev, n_people_dev, scene_id_dev, batch, max_people, h,
                           w, n_samples, flags, noise_sigma, seed, static_cast<__half *>(out_dev), (int)tiles_x, vec);
    else
        hipLaunchKernelGGL(k_render_scenes<float>, grid, block, lds, st, joints_dev, n_people_dev, scene_id_dev, batch, max_people, h,
                           w, n_samples, flags, noise_sigma, seed, static_cast<float *>(out_dev), (int)tiles_x, vec);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
