// posepaf_augment.hip -- the training-data transformer of the reference (py_cocodata_server/py_data_transformer.py:42-88, :111-183,
// py_data_iterator.py:54-74, py_data_heatmapper.py:79-86) as one device stage: uint8 slots in, (image, mask_miss, foreground,
// joints) out.  The arithmetic is the CONTRACT of INTEGRATION section 17 (it follows OpenCV 3.4 imgwarp.cpp / resize.cpp /
// morph.cpp, but it is that statement, restated in tests/augment_reference.py, the kernels are held to -- not a cv2 run):
//   coordinates  as posepaf_affine.h: X = (rint((M1 y + M2) 1024) + 16 + rint(M0 x 1024)) >> 5, Y likewise; sx = X >> 5, fx = X & 31
//   bilinear     all integer, a = fx, b = fy: v = (v00 (32-a)(32-b) + v01 a (32-b) + v10 (32-a) b + v11 a b + 512) >> 10
//   border       BORDER_CONSTANT: every tap outside the (h_b, w_b) source reads the border value (image border[c], mask_miss 255,
//                mask_all 0); four outside taps give exactly the border value, so a block wholly outside needs no case of its own
//   masks        to stride 4 (INTER_AREA, factor 4): m = rint_half_even(sum of the 4 x 4 warped values / 16), stored float(m) / 255.0f
//   foreground   cv2.erode 3 x 3 of the stride-4 mask_all: the minimum over the neighbours inside the frame
//   image        float(u8) / 255.0f, a correctly rounded division (a 256-entry table of __fdiv_rn in LDS); fp16 = that value rounded
//   joints       x' = (m0 x + m1 y) + m2 in float64, every operation rounded on its own, then rounded to float32; after a flip the
//                left and right parts exchange whole rows
// k_augment_warp: a workgroup takes 16 x 16 cells (64 x 64 destination pixels) of one image.  A wave works on one 16 x 4 pixel patch
// at a time, a lane on one pixel: its tap is computed once and serves the image and both masks.  A rotated read puts distant
// destination pixels on different source lines, so the patch is kept compact (a wave instruction touches about a dozen lines, not
// 64) and the two taps of a source row travel in ONE load of any alignment: 8 bytes of the image, 2 of a mask plane -- 6 loads per
// pixel, not 20.  A lane stores its pixel's 12 bytes (fp32; fp16: lane pairs store their 12), 768 contiguous bytes per patch row.
// The 4 x 4 cell sums of both masks are formed by four xor-shuffles on one packed word and go to LDS; after a barrier one lane per
// cell rounds, divides and stores mask_miss and takes the 3 x 3 minimum of mask_all.  The 68 cells of the ring around the block
// are recomputed (mask_all only), 16 lanes per cell.  No atomics, no scratch, nothing that depends on the launch geometry, the batch
// composition or the slot.  Every per-image parameter is read from device memory.
// The sums X0 + adelta are formed in unsigned arithmetic and every tap is bounds-checked against the source, so a matrix beyond the
// documented range gives wrong pixels, never an address outside the slot.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "posepaf_affine.h"
#include "posepaf_internal.h"

namespace {

constexpr int AG_C = 16;                 // cells per block side
constexpr int AG_THREADS = AG_C * AG_C;
constexpr int AG_HALO = AG_C + 2;
constexpr int AG_NHALO = 4 * AG_C + 4;   // 68 ring cells
constexpr int AG_OUTSIDE = 256;          // a cell outside the frame: above every uint8, so a minimum never picks it

struct AugArgs {
    const unsigned char *img, *miss, *all;
    const int *sizes;
    const double *m_inv;
    int batch, slot_h, slot_w, out_h, out_w;
    unsigned char border[4];
    void *image_out;
    float *miss_out;
    void *fg_out;
    int fg_f16;
    long long fg_stride;
};

struct Tap {
    int sx, sy, w00, w01, w10, w11;
};

__device__ __forceinline__ Tap make_tap(int2 row, int2 col) {
    const int X = (int)((unsigned)row.x + (unsigned)col.x) >> 5, Y = (int)((unsigned)row.y + (unsigned)col.y) >> 5;
    Tap t;
    t.sx = X >> 5, t.sy = Y >> 5;
    const int a = X & 31, b = Y & 31;
    t.w00 = (32 - a) * (32 - b), t.w01 = a * (32 - b), t.w10 = (32 - a) * b, t.w11 = a * b;
    return t;
}

__device__ __forceinline__ int blend(const Tap &t, int v00, int v01, int v10, int v11) {
    return (v00 * t.w00 + v01 * t.w01 + v10 * t.w10 + v11 * t.w11 + 512) >> 10;
}

// the two taps of a source row as one load of any alignment (global loads need none on gfx950)
__device__ __forceinline__ unsigned load2(const unsigned char *p) {
    unsigned short v;
    __builtin_memcpy(&v, p, 2);
    return v;
}
__device__ __forceinline__ unsigned long long load8(const unsigned char *p) {
    unsigned long long v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// one warped value of a single-channel plane (row stride slot_w) with a constant border
__device__ __forceinline__ int warp_plane(const unsigned char *plane, int slot_w, int h, int w, const Tap &t, int border) {
    const bool x0 = t.sx >= 0 && t.sx < w, x1 = t.sx + 1 >= 0 && t.sx + 1 < w;
    const bool y0 = t.sy >= 0 && t.sy < h, y1 = t.sy + 1 >= 0 && t.sy + 1 < h;
    const unsigned char *p = plane + (long long)t.sy * slot_w + t.sx;       // dereferenced only where the tap is inside
    if (x0 && x1 && y0 && y1) {
        const unsigned top = load2(p), bot = load2(p + slot_w);
        return blend(t, top & 255, top >> 8, bot & 255, bot >> 8);
    }
    const int v00 = (y0 && x0) ? p[0] : border, v01 = (y0 && x1) ? p[1] : border;
    const int v10 = (y1 && x0) ? p[slot_w] : border, v11 = (y1 && x1) ? p[slot_w + 1] : border;
    return blend(t, v00, v01, v10, v11);
}

// the three warped channels of one image pixel
__device__ __forceinline__ void warp_image(const unsigned char *img, int slot_w, int h, int w, const Tap &t, const int border[3],
                                           int v[3]) {
    const bool x0 = t.sx >= 0 && t.sx < w, x1 = t.sx + 1 >= 0 && t.sx + 1 < w;
    const bool y0 = t.sy >= 0 && t.sy < h, y1 = t.sy + 1 >= 0 && t.sy + 1 < h;
    const unsigned char *p = img + ((long long)t.sy * slot_w + t.sx) * 3, *q = p + (long long)slot_w * 3;
    if (x0 && x1 && y0 && y1 && t.sx + 2 < w) {                    // bytes 3 sx .. 3 sx + 7 lie inside the image's own rows
        const unsigned long long top = load8(p), bot = load8(q);
#pragma unroll
        for (int c = 0; c < 3; c++)
            v[c] = blend(t, (int)(top >> (8 * c)) & 255, (int)(top >> (24 + 8 * c)) & 255, (int)(bot >> (8 * c)) & 255,
                         (int)(bot >> (24 + 8 * c)) & 255);
        return;
    }
    const bool i00 = y0 && x0, i01 = y0 && x1, i10 = y1 && x0, i11 = y1 && x1;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int bd = border[c];
        v[c] = blend(t, i00 ? p[c] : bd, i01 ? p[3 + c] : bd, i10 ? q[c] : bd, i11 ? q[3 + c] : bd);
    }
}

// rint_half_even(sum / 16) of a sum of 16 uint8 values
__device__ __forceinline__ int round16(int sum) { return (sum + 7 + ((sum >> 4) & 1)) >> 4; }

struct alignas(4) Float3 {
    float v[3];
};

// one pixel's three values to dst (the pixel's first element).  fp16: the lane pair (2 i, 2 i + 1) holds 12 contiguous bytes; the
// even lane stores the first 8, the odd lane the last 4 (both lanes of a pair are active together: a cell is 4 pixels wide)
template <typename T>
__device__ __forceinline__ void store_pixel(T *dst, const float v[3], bool active);
template <>
__device__ __forceinline__ void store_pixel<float>(float *dst, const float v[3], bool active) {
    if (active) *reinterpret_cast<Float3 *>(dst) = Float3{{v[0], v[1], v[2]}};
}
template <>
__device__ __forceinline__ void store_pixel<__half>(__half *dst, const float v[3], bool active) {
    const unsigned h0 = __half_as_ushort(__float2half_rn(v[0])), h1 = __half_as_ushort(__float2half_rn(v[1]));
    const unsigned h2 = __half_as_ushort(__float2half_rn(v[2]));
    const unsigned other0 = (unsigned)__shfl_xor((int)h0, 1);    // every lane takes part
    if (!active) return;
    if ((threadIdx.x & 1) == 0) {
        unsigned *d = reinterpret_cast<unsigned *>(dst);          // 12-byte aligned from a 16-byte aligned base: 4-byte aligned
        d[0] = h0 | (h1 << 16);
        d[1] = h2 | (other0 << 16);
    } else {
        *reinterpret_cast<unsigned *>(dst + 1) = h1 | (h2 << 16);
    }
}

template <typename T>
__global__ __launch_bounds__(AG_THREADS) void k_augment_warp(AugArgs a) {
    __shared__ float s_lut[256];                    // u / 255.0f, correctly rounded
    __shared__ int s_all[AG_HALO * AG_HALO];        // 4 x 4 sums of mask_all of the block's cells and its ring, -1 outside the frame
    __shared__ int s_miss[AG_C * AG_C];             // 4 x 4 sums of mask_miss of the block's cells
    const int tid = threadIdx.x, b = blockIdx.z;
    const int wave = tid >> 6, lane = tid & 63, lx = lane & 15, ly = lane >> 4;
    const int cw = a.out_w >> 2, ch = a.out_h >> 2;
    s_lut[tid] = __fdiv_rn((float)tid, 255.0f);

    int h = a.slot_h, w = a.slot_w;
    if (a.sizes) {
        h = min(max(a.sizes[b], 0), a.slot_h);
        w = min(max(a.sizes[a.batch + b], 0), a.slot_w);
    }
    double m[6];
#pragma unroll
    for (int i = 0; i < 6; i++) m[i] = a.m_inv[6 * b + i];
    const long long slot = (long long)b * a.slot_h * a.slot_w;
    const unsigned char *img = a.img + slot * 3;
    const unsigned char *miss = a.miss ? a.miss + slot : nullptr;
    const unsigned char *all = a.all ? a.all + slot : nullptr;
    const int border[3] = {a.border[0], a.border[1], a.border[2]};
    __syncthreads();                                // the table

    // ---- the block's 64 x 64 pixels: wave `wave` takes rows 16 wave .. + 15 as 4 x 4 patches of 16 x 4 pixels
    const int x0 = (int)blockIdx.x * 4 * AG_C, y0 = (int)blockIdx.y * 4 * AG_C + 16 * wave;
    int2 col[4];
#pragma unroll
    for (int j = 0; j < 4; j++) col[j] = pp::affine_col(m, x0 + 16 * j + lx);
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const int y = y0 + 4 * k + ly;
        const int2 row = pp::affine_row(m, y);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = x0 + 16 * j + lx;
            const bool active = x < a.out_w && y < a.out_h;
            float v[3] = {0.0f, 0.0f, 0.0f};
            int packed = 0;                          // mask_miss | mask_all << 16
            if (active) {
                const Tap t = make_tap(row, col[j]);
                int u[3];
                warp_image(img, a.slot_w, h, w, t, border, u);
                v[0] = s_lut[u[0]], v[1] = s_lut[u[1]], v[2] = s_lut[u[2]];
                packed = miss ? warp_plane(miss, a.slot_w, h, w, t, 255) : 255;
                if (all) packed |= warp_plane(all, a.slot_w, h, w, t, 0) << 16;
            }
            store_pixel<T>(static_cast<T *>(a.image_out) + (((long long)b * a.out_h + y) * a.out_w + x) * 3, v, active);
            // the cell's 16 pixels: lanes lx ^ {1, 2} and ly ^ {1, 2}; each half stays below 2^16
            packed += __shfl_xor(packed, 1);
            packed += __shfl_xor(packed, 2);
            packed += __shfl_xor(packed, 16);
            packed += __shfl_xor(packed, 32);
            if (lane == (lx & 12)) {                 // ly = 0 and lx a multiple of 4: one lane per cell
                const int cxl = 4 * j + (lx >> 2), cyl = 4 * wave + k;
                s_miss[cyl * AG_C + cxl] = packed & 0xFFFF;
                s_all[(cyl + 1) * AG_HALO + cxl + 1] = active ? packed >> 16 : -1;
            }
        }
    }

    // ---- the ring of 68 cells around the block, mask_all only: 16 lanes per cell
    if (all) {                                      // uniform over the launch
#pragma unroll 1
        for (int q = tid; q < ((AG_NHALO * 16 + AG_THREADS - 1) / AG_THREADS) * AG_THREADS; q += AG_THREADS) {
            const int rc = q >> 4, px = q & 3, py = (q >> 2) & 3;
            int hx = 0, hy = 0;
            if (rc < AG_HALO) hx = rc, hy = 0;
            else if (rc < 2 * AG_HALO) hx = rc - AG_HALO, hy = AG_HALO - 1;
            else if (rc < 2 * AG_HALO + AG_C) hx = 0, hy = rc - 2 * AG_HALO + 1;
            else hx = AG_HALO - 1, hy = rc - 2 * AG_HALO - AG_C + 1;
            const int gx = (int)blockIdx.x * AG_C + hx - 1, gy = (int)blockIdx.y * AG_C + hy - 1;
            const bool inside = rc < AG_NHALO && gx >= 0 && gx < cw && gy >= 0 && gy < ch;
            int sum = 0;
            if (inside) sum = warp_plane(all, a.slot_w, h, w, make_tap(pp::affine_row(m, 4 * gy + py), pp::affine_col(m, 4 * gx + px)), 0);
            sum += __shfl_xor(sum, 1);
            sum += __shfl_xor(sum, 2);
            sum += __shfl_xor(sum, 4);
            sum += __shfl_xor(sum, 8);
            if ((q & 15) == 0 && rc < AG_NHALO) s_all[hy * AG_HALO + hx] = inside ? sum : -1;
        }
    }
    __syncthreads();

    // ---- one lane per cell: mask_miss, and the erode -- the 3 x 3 minimum over the cells inside the frame
    const int clx = tid & (AG_C - 1), cly = tid >> 4;
    const int cx = (int)blockIdx.x * AG_C + clx, cy = (int)blockIdx.y * AG_C + cly;
    if (cx >= cw || cy >= ch) return;
    a.miss_out[((long long)b * ch + cy) * cw + cx] = s_lut[round16(s_miss[tid])];
    float fg = 0.0f;
    if (all) {
        int mn = AG_OUTSIDE;
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
            for (int dx = 0; dx < 3; dx++) {
                const int s = s_all[(cly + dy) * AG_HALO + clx + dx];
                if (s >= 0) mn = min(mn, round16(s));
            }
        fg = s_lut[mn];                              // the cell itself is inside the frame: mn <= 255
    }
    const long long o = (long long)b * a.fg_stride + (long long)cy * cw + cx;
    if (a.fg_f16) static_cast<__half *>(a.fg_out)[o] = __float2half_rn(fg);
    else static_cast<float *>(a.fg_out)[o] = fg;
}

// the part whose row a part takes after a flip: leftParts <-> rightParts of the reference's 18-part order
__device__ const int8_t d_flip_part[PP_NUM_PART] = {0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16};

__global__ __launch_bounds__(256) void k_augment_joints(const double *__restrict__ jin, const int *__restrict__ n_people,
                                                        const double *__restrict__ m_fwd, const int *__restrict__ flip, int max_people,
                                                        float *__restrict__ jout) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;          // (person, part)
    if (i >= max_people * PP_NUM_PART) return;
    const int p = i / PP_NUM_PART, k = i - p * PP_NUM_PART;
    const long long base = ((long long)b * max_people + p) * PP_NUM_PART;
    float *o = jout + (base + k) * 3;
    if (p >= min(max(n_people[b], 0), max_people)) {        // written as it was
        const double *s = jin + (base + k) * 3;
        o[0] = __double2float_rn(s[0]), o[1] = __double2float_rn(s[1]), o[2] = __double2float_rn(s[2]);
        return;
    }
    const double *s = jin + (base + (flip[b] ? d_flip_part[k] : k)) * 3;
    const double *m = m_fwd + 6 * b;
    const double x = s[0], y = s[1];
    o[0] = __double2float_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], x), __dmul_rn(m[1], y)), m[2]));
    o[1] = __double2float_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[3], x), __dmul_rn(m[4], y)), m[5]));
    o[2] = __double2float_rn(s[2]);
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

extern "C" int pp_augment_batch(const void *images_u8, const int *sizes_dev, const void *mask_miss_u8, const void *mask_all_u8, int batch,
                                int slot_h, int slot_w, const double *m_inv_dev, const double *m_fwd_dev, const int *flip_dev,
                                const double *joints_in_dev, const int *n_people_dev, int max_people, int out_h, int out_w,
                                const unsigned char *border, void *image_out, int image_dtype, float *mask_miss_out, void *fg_out,
                                int fg_dtype, long long fg_image_stride, float *joints_out, void *stream) {
    if (!images_u8 || !m_inv_dev || !m_fwd_dev || !flip_dev || !joints_in_dev || !n_people_dev || !border || !image_out ||
        !mask_miss_out || !fg_out || !joints_out)
        return PP_ERR_BAD_ARG;
    if (batch <= 0 || slot_h <= 0 || slot_w <= 0 || max_people <= 0 || out_h <= 0 || out_w <= 0 || (out_h & 3) || (out_w & 3))
        return PP_ERR_BAD_ARG;
    if ((image_dtype != PP_F16 && image_dtype != PP_F32) || (fg_dtype != PP_F16 && fg_dtype != PP_F32)) return PP_ERR_BAD_ARG;
    if (fg_image_stride < (long long)(out_h / 4) * (out_w / 4)) return PP_ERR_BAD_ARG;
    // image_out on a 16-byte boundary: a pixel's 12 (fp32) bytes and a pixel pair's 12 (fp16) bytes are then 4-byte aligned stores
    if (reinterpret_cast<uintptr_t>(image_out) % 16 || reinterpret_cast<uintptr_t>(mask_miss_out) % 4 ||
        reinterpret_cast<uintptr_t>(fg_out) % (fg_dtype == PP_F16 ? 2 : 4) || reinterpret_cast<uintptr_t>(joints_out) % 4 ||
        reinterpret_cast<uintptr_t>(m_inv_dev) % 8 || reinterpret_cast<uintptr_t>(m_fwd_dev) % 8 ||
        reinterpret_cast<uintptr_t>(joints_in_dev) % 8)
        return PP_ERR_BAD_ARG;
    if (max_people > PP_SCENE_MAX_PEOPLE) return PP_ERR_UNSUPPORTED;
    if (batch > 65535 || slot_h > 32768 || slot_w > 32768 || out_h > 32768 || out_w > 32768) return PP_ERR_TOO_LARGE;
    if (!device_present()) return PP_ERR_NO_DEVICE;
    AugArgs a;
    a.img = static_cast<const unsigned char *>(images_u8);
    a.miss = static_cast<const unsigned char *>(mask_miss_u8);
    a.all = static_cast<const unsigned char *>(mask_all_u8);
    a.sizes = sizes_dev;
    a.m_inv = m_inv_dev;
    a.batch = batch, a.slot_h = slot_h, a.slot_w = slot_w, a.out_h = out_h, a.out_w = out_w;
    a.border[0] = border[0], a.border[1] = border[1], a.border[2] = border[2], a.border[3] = 0;
    a.image_out = image_out, a.miss_out = mask_miss_out, a.fg_out = fg_out;
    a.fg_f16 = fg_dtype == PP_F16, a.fg_stride = fg_image_stride;
    const int cw = out_w / 4, ch = out_h / 4;
    const dim3 grid((unsigned)((cw + AG_C - 1) / AG_C), (unsigned)((ch + AG_C - 1) / AG_C), (unsigned)batch), block(AG_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (image_dtype == PP_F16) hipLaunchKernelGGL(k_augment_warp<__half>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_augment_warp<float>, grid, block, 0, st, a);
    const dim3 jgrid((unsigned)((max_people * PP_NUM_PART + 255) / 256), (unsigned)batch);
    hipLaunchKernelGGL(k_augment_joints, jgrid, dim3(256), 0, st, joints_in_dev, n_people_dev, m_fwd_dev, flip_dev, max_people, joints_out);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
