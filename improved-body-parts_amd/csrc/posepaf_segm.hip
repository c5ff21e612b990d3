// posepaf_segm.hip -- the person masks of the reference's data/coco_masks_hdf5.py (make_mask over pycocotools' annToMask) written on
// the device from polygon vertices and one uncompressed crowd run-length code per image: mask_miss and mask_all, uint8, in the slots
// pp_augment_batch reads.  The arithmetic is the CONTRACT of INTEGRATION section 19 (it follows the published maskApi.c: rleFrPoly,
// rleMerge, rleDecode; tests/coco_mask_reference.py restates it), not a pycocotools run:
//   vertices   X = (int)(5.0 x + 0.5), float64, every operation rounded on its own (k_segm_vertices, once per launch, into the workspace)
//   edge       dx = |Xb - Xa|, dy = |Yb - Ya|; rleFrPoly walks max(dx, dy) + 1 dense points (u, v) and every consecutive pair with
//              different u whose smaller u is 5 x + 2 is an event of column x, at y = ceil(clamp((min(v) + 0.5) / 5.0 - 0.5, 0, h))
//   ring       pixel (x, y) is 1 iff an odd number of column x's events have y_e <= y;  annotations, crowd and make_mask's
//              combination are ORs and one AND NOT of such planes
// The dense points are never materialised.  An edge crosses a column's boundary (u from 5 x + 2 to 5 x + 3) at most once, and the pair
// of points on either side is found in closed form: for dx >= dy its two v are two evaluations of the literal (int)(Ya + s t + 0.5);
// for dx < dy the first t whose u reaches the boundary is estimated by a division and then corrected against the literal
// (int)(Xa + s t + 0.5), which is monotone in t.  So the cost follows the columns an edge spans, not the points it would emit, and no
// event list, sort or atomic on a mask byte exists.
// k_segm_masks: a workgroup takes 256 columns x 64 rows of one image, a thread one column with its 64 rows as bits of one word.  Per
// ring the threads share the edges, toggle bit max(y_e - y0, 0) of the column's word in LDS (atomic xor: only the parity of a count
// matters, so the order does not), and after one barrier each thread turns its word into the column's parity by a prefix xor and ORs
// it into the planes the ring counts for.  Two LDS buffers alternate so that one barrier per ring suffices.  The crowd's runs are
// prefix sums over the column-major pixel order p = x h + y: a binary search finds the run of the column's first row.  The finished
// words are transposed through LDS and stored as 16-byte row segments where the address allows it, bytes elsewhere; nothing outside
// (h_b, w_b) is written.  Every table entry read from device memory is clamped against the counts given on the host, so a wrong
// table gives wrong pixels, never an address outside the buffers.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "posepaf_internal.h"

namespace {

constexpr int SG_COLS = 256, SG_ROWS = 64, SG_THREADS = 256;
constexpr int SG_COORD_LIMIT = 1 << 27;         // 5 * 2^24 + 1 lies below it: differences of two coordinates stay in int
constexpr int SG_MAX_RINGS = 1 << 20, SG_MAX_VERTS = 1 << 24, SG_MAX_RUNS = 1 << 24;

struct SegmArgs {
    const int2 *vert;
    const int4 *rings;
    const long long *images, *runs;
    const int *sizes;
    int batch, slot_h, slot_w, n_rings, n_verts, n_runs;
    unsigned char *miss, *all;
};

__global__ __launch_bounds__(256) void k_segm_vertices(const double *__restrict__ xy, int n, int2 *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(5.0 * xy[2 * i] + 0.5), y = (int)(5.0 * xy[2 * i + 1] + 0.5);
    out[i] = make_int2(min(max(x, -SG_COORD_LIMIT), SG_COORD_LIMIT), min(max(y, -SG_COORD_LIMIT), SG_COORD_LIMIT));
}

__device__ __forceinline__ int floor_div5(int v) { return v >= 0 ? v / 5 : -((4 - v) / 5); }

// the event of a pair of dense points whose smaller v is yraw, in the column with local index c
__device__ __forceinline__ void toggle(unsigned (*tog)[2], int c, int yraw, int h, int y0) {
    double yd = ((double)yraw + 0.5) / 5.0 - 0.5;
    if (yd < 0.0) yd = 0.0;
    else if (yd > (double)h) yd = (double)h;
    const int bit = max((int)ceil(yd) - y0, 0);
    if (bit < SG_ROWS) atomicXor(&tog[c][bit >> 5], 1u << (bit & 31));
}

// the events of edge a -> b in the columns x0 .. x_last (inside the frame)
__device__ __forceinline__ void emit_edge(unsigned (*tog)[2], int2 a, int2 b, int x0, int x_last, int h, int y0) {
    const int dx = abs(b.x - a.x), dy = abs(b.y - a.y);
    if (dx == 0) return;                                   // u never changes (and the 0 / 0 edge of the C source)
    // columns c with lo <= 5 c + 2 and 5 c + 3 <= hi
    const int c_lo = max(floor_div5(min(a.x, b.x) + 2), x0), c_hi = min(floor_div5(max(a.x, b.x) - 3), x_last);
    if (dx >= dy) {
        const int xs = min(a.x, b.x), ys = a.x < b.x ? a.y : b.y, ye = a.x < b.x ? b.y : a.y;
        const double s = (double)(ye - ys) / (double)dx;
        for (int c = c_lo; c <= c_hi; c++) {
            const int t = 5 * c + 2 - xs;
            const int v0 = (int)((double)ys + s * (double)t + 0.5), v1 = (int)((double)ys + s * (double)(t + 1) + 0.5);
            toggle(tog, c - x0, min(v0, v1), h, y0);
        }
    } else {
        const int ys = min(a.y, b.y), xs = a.y < b.y ? a.x : b.x, xe = a.y < b.y ? b.x : a.x;
        const double s = (double)(xe - xs) / (double)dy;
        const bool up = xe > xs;
        for (int c = c_lo; c <= c_hi; c++) {
            // the first t in 1 .. dy whose u has crossed: u(t) >= 5 c + 3 going up, u(t) <= 5 c + 2 going down; u(t - 1) is the other
            const int T = up ? 5 * c + 3 : 5 * c + 2;
            int t = (int)(((double)T - (double)xs) / s);
            t = min(max(t, 1), dy);
            auto crossed = [&](int tt) {
                const int u = (int)((double)xs + s * (double)tt + 0.5);
                return up ? u >= T : u <= T;
            };
            while (t > 1 && crossed(t - 1)) t--;
            while (t < dy && !crossed(t)) t++;
            toggle(tog, c - x0, ys + t - 1, h, y0);
        }
    }
}

__device__ __forceinline__ int fin_index(int col) { return col + (col >> 4); }   // 16 lanes 16 columns apart: 16 different banks

__global__ __launch_bounds__(SG_THREADS) void k_segm_masks(SegmArgs a) {
    __shared__ unsigned s_tog[2][SG_COLS][2];
    __shared__ unsigned long long s_fin[2][SG_COLS + SG_COLS / 16];
    const int tid = threadIdx.x, b = blockIdx.z;
    int h = a.slot_h, w = a.slot_w;
    if (a.sizes) {
        h = min(max(a.sizes[b], 0), a.slot_h);
        w = min(max(a.sizes[a.batch + b], 0), a.slot_w);
    }
    const int x0 = (int)blockIdx.x * SG_COLS, y0 = (int)blockIdx.y * SG_ROWS;
    if (x0 >= w || y0 >= h) return;                         // uniform over the workgroup
    s_tog[0][tid][0] = s_tog[0][tid][1] = s_tog[1][tid][0] = s_tog[1][tid][1] = 0;
    __syncthreads();

    const long long *im = a.images + 5 * (long long)b;
    const int ring_first = (int)min(max(im[0], 0LL), (long long)a.n_rings);
    const int ring_count = (int)min(max(im[1], 0LL), (long long)(a.n_rings - ring_first));
    const int run_first = (int)min(max(im[2], 0LL), (long long)a.n_runs);
    const int run_count = (int)min(max(im[3], 0LL), (long long)(a.n_runs - run_first));
    const long long crowd_order = im[4];
    const int x_last = min(x0 + SG_COLS, w) - 1;

    unsigned long long acc_all = 0, acc_miss = 0, acc_before = 0;
    int buf = 0;
    for (int r = ring_first; r < ring_first + ring_count; r++) {
        const int4 ring = a.rings[r];                       // first vertex, vertices, order index, flags
        if (ring.x < 0 || ring.y < 3 || ring.y > a.n_verts || ring.x > a.n_verts - ring.y) continue;    // uniform
        const int2 *v = a.vert + ring.x;
        for (int j = tid; j < ring.y; j += SG_THREADS) emit_edge(s_tog[buf], v[j], v[j + 1 == ring.y ? 0 : j + 1], x0, x_last, h, y0);
        __syncthreads();
        unsigned long long m = s_tog[buf][tid][0] | ((unsigned long long)s_tog[buf][tid][1] << 32);
        s_tog[buf][tid][0] = s_tog[buf][tid][1] = 0;        // for the ring after the next; a barrier lies in between
        m ^= m << 1, m ^= m << 2, m ^= m << 4, m ^= m << 8, m ^= m << 16, m ^= m << 32;
        acc_all |= m;
        if (ring.w & 1) acc_miss |= m;
        if (run_count > 0 && ring.z < crowd_order) acc_before |= m;
        buf ^= 1;
    }

    // the crowd: run i covers the pixels cum[i - 1] .. cum[i] - 1 of the column-major order and is set when i is odd
    unsigned long long crowd = 0;
    const int x = x0 + tid, rows = min(SG_ROWS, h - y0);
    if (run_count > 0 && x < w) {
        const long long *cum = a.runs + run_first;
        const long long p0 = (long long)x * h + y0, p_end = p0 + rows;
        int lo = 0, hi = run_count;                         // the first run that ends behind p0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] > p0) hi = mid;
            else lo = mid + 1;
        }
        long long p = p0;
        for (int i = lo; i < run_count && p < p_end; i++) {
            const long long e = min(cum[i], p_end);
            if (e <= p) continue;
            const int n = (int)(e - p);
            if (i & 1) crowd |= (n == 64 ? ~0ULL : ((1ULL << n) - 1)) << (int)(p - p0);
            p = e;
        }
    }
    crowd &= ~acc_before;
    s_fin[0][fin_index(tid)] = ~(acc_miss | crowd);
    s_fin[1][fin_index(tid)] = acc_all | crowd;
    __syncthreads();

    // rows of 16 columns: one 16-byte store where the address allows it
    for (int seg = tid; seg < SG_ROWS * (SG_COLS / 16); seg += SG_THREADS) {
        const int row = seg >> 4, cs = (seg & 15) * 16;
        if (row >= rows || x0 + cs >= w) continue;
        const int n = min(16, w - x0 - cs);
        const long long o = ((long long)b * a.slot_h + y0 + row) * a.slot_w + x0 + cs;
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
            unsigned word[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 16; i++)
                if ((s_fin[pl][fin_index(cs + i)] >> row) & 1) word[i >> 2] |= 255u << (8 * (i & 3));
            unsigned char *dst = (pl ? a.all : a.miss) + o;
            if (n == 16 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4(word[0], word[1], word[2], word[3]);
            } else {
                for (int i = 0; i < n; i++) dst[i] = (unsigned char)(word[i >> 2] >> (8 * (i & 3)));
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

extern "C" long long pp_coco_masks_workspace_bytes(int n_verts) {
    if (n_verts < 0) return PP_ERR_BAD_ARG;
    if (n_verts > SG_MAX_VERTS) return PP_ERR_TOO_LARGE;
    return (long long)sizeof(int2) * (n_verts > 0 ? n_verts : 1);
}

extern "C" int pp_coco_masks_u8(const double *verts_dev, int n_verts, const int *rings_dev, int n_rings, const long long *images_dev,
                                const long long *runs_dev, int n_runs, const int *sizes_dev, int batch, int slot_h, int slot_w,
                                void *workspace, long long workspace_bytes, void *mask_miss_u8, void *mask_all_u8, void *stream) {
    if (!images_dev || !workspace || !mask_miss_u8 || !mask_all_u8 || mask_miss_u8 == mask_all_u8) return PP_ERR_BAD_ARG;
    if (batch <= 0 || slot_h <= 0 || slot_w <= 0 || n_verts < 0 || n_rings < 0 || n_runs < 0) return PP_ERR_BAD_ARG;
    if ((n_verts > 0 && !verts_dev) || (n_rings > 0 && !rings_dev) || (n_runs > 0 && !runs_dev)) return PP_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(verts_dev) % 8 || reinterpret_cast<uintptr_t>(rings_dev) % 16 ||
        reinterpret_cast<uintptr_t>(images_dev) % 8 || reinterpret_cast<uintptr_t>(runs_dev) % 8 ||
        reinterpret_cast<uintptr_t>(sizes_dev) % 4 || reinterpret_cast<uintptr_t>(workspace) % 8)
        return PP_ERR_BAD_ARG;
    if (batch > 65535 || slot_h > 32768 || slot_w > 32768 || n_verts > SG_MAX_VERTS || n_rings > SG_MAX_RINGS || n_runs > SG_MAX_RUNS)
        return PP_ERR_TOO_LARGE;
    if (workspace_bytes < pp_coco_masks_workspace_bytes(n_verts)) return PP_ERR_BAD_ARG;
    if (!device_present()) return PP_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_verts > 0)
        hipLaunchKernelGGL(k_segm_vertices, dim3((unsigned)((n_verts + 255) / 256)), dim3(256), 0, st, verts_dev, n_verts,
                           static_cast<int2 *>(workspace));
    SegmArgs a;
    a.vert = static_cast<const int2 *>(workspace);
    a.rings = reinterpret_cast<const int4 *>(rings_dev);
    a.images = images_dev, a.runs = runs_dev, a.sizes = sizes_dev;
    a.batch = batch, a.slot_h = slot_h, a.slot_w = slot_w, a.n_rings = n_rings, a.n_verts = n_verts, a.n_runs = n_runs;
    a.miss = static_cast<unsigned char *>(mask_miss_u8), a.all = static_cast<unsigned char *>(mask_all_u8);
    const dim3 grid((unsigned)((slot_w + SG_COLS - 1) / SG_COLS), (unsigned)((slot_h + SG_ROWS - 1) / SG_ROWS), (unsigned)batch);
    hipLaunchKernelGGL(k_segm_masks, grid, dim3(SG_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
