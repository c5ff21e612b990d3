// posepaf_internal.h -- declarations shared by the kernels and the C-ABI host code (not installed).
#ifndef POSEPAF_INTERNAL_H
#define POSEPAF_INTERNAL_H

#include <hip/hip_runtime.h>

#include "../../include/posepaf.h"

// The skeleton's tables, ONE copy of the values for every translation unit that needs them on the device (each defines its own
// __device__ array from the list: the library is built without relocatable device code).
// limbs: utils/pafprocess/pafprocess.h:21-27 (== config/config.py:114-121); flip orders: config/config.py:150-152
#define PP_LIMB_FROM_LIST {1, 1, 1, 1, 1, 0, 0, 14, 15, 1, 2, 3, 1, 5, 6, 1, 8, 9, 1, 11, 12, 0, 0, 2, 8, 5, 11, 16, 17, 8}
#define PP_LIMB_TO_LIST {0, 14, 15, 16, 17, 14, 15, 16, 17, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 2, 5, 8, 12, 11, 9, 2, 5, 11}
#define PP_FLIP_HEAT_ORD_LIST {0, 1, 5, 6, 7, 2, 3, 4, 11, 12, 13, 8, 9, 10, 15, 14, 17, 16, 18, 19}
#define PP_FLIP_PAF_ORD_LIST \
    {0, 2, 1, 4, 3, 6, 5, 8, 7, 12, 13, 14, 9, 10, 11, 18, 19, 20, 15, 16, 17, 22, 21, 25, 26, 23, 24, 28, 27, 29}

namespace pp {

// 160 KiB of LDS per CU (gfx950) minus room for the kernels' static __shared__ arrays (< 2 KB)
constexpr size_t kMaxDynLds = 163840 - 4096;
hipError_t init_kernel_attributes();
hipError_t set_stamp_buffer(long long *buf);

// status flag words per image: [0, 18) one per part (peak kernels), [18, 48) one per limb (limb kernels); see or_flags
constexpr int kFlagWordsPerImage = PP_NUM_PART + PP_NUM_LIMB;

size_t lds_bytes_heat(int elem, int h, int w, int maxp);
size_t lds_bytes_limb(int elem, int h, int w, int maxp, int cap);
size_t lds_bytes_limb_hwc(int maxp, int cap);
size_t lds_bytes_assemble(int maxp);

// Where K_A / K_B read the feature map of shape (h, w) and element type dtype.  !hbm: ptr is the caller's network output
// (batch, n_samples, 50, h, w), which the kernels flip-average into LDS themselves.  hbm: ptr is the workspace
// ws[batch][48][ws_stride] that launch_flip_average_maps filled from it (maps larger than LDS); the
// launchers then run the _hbm instances, which read it in place.
struct MapSource {
    bool hbm;
    const void *ptr;
    int dtype, h, w;
    int n_samples, flip;   // of the network output (the kernels read them only when !hbm)
    size_t ws_stride;      // hbm only: elements per plane (map_plane_stride)
};
constexpr size_t kMaxHbmPixels = (size_t)650 * 950;   // the reference's own cap on this path (utils/parse_skeletons.py:46-49), / 4
size_t lds_bytes_heat_hbm(int h, int w, int maxp, int batch);
size_t lds_bytes_limb_hbm(int maxp, int cap);
size_t map_plane_stride(int elem, int h, int w);    // elements: h*w rounded up to 16 bytes
size_t map_workspace_bytes(int batch, int h, int w);  // batch * 48 planes of fp32 + 16 bytes of slack
hipError_t launch_flip_average_maps(const void *net, int dtype, int batch, int n_samples, int h, int w, int flip, void *ws,
                                    hipStream_t stream);
// order / arrive_all (both or neither): K_A's last workgroup writes the images sorted by matching load into order[batch]
hipError_t launch_heat_peaks(const MapSource &src, int batch, int refine, int nms_mode, float thr, int maxp, float4 *peaks,
                             int *counts, unsigned *status, int *order, int *arrive_all, hipStream_t stream);
bool heat_peaks_sorts(int dtype, int batch, int h, int w, int maxp);
// arrive != NULL: fused form, workgroup 30 of each image assembles it into records WHILE its limbs are matched (arrive[batch]:
// per-image launch counters, ready[batch][30]: per-limb publication flags; both zeroed once at create and owned by the kernel);
// arrive == NULL: connections only (launch_assemble_wave follows).  order may be NULL.
hipError_t launch_limb_connect(const MapSource &src, int batch, int maxp, int cap, int min_img_size, const int *min_img_size_dev,
                               const float4 *peaks, const int *counts, float4 *conns, float4 *aux, int *conn_counts,
                               unsigned *status, const int *order, int *arrive, unsigned *ready, pp_record *records,
                               hipStream_t stream);
hipError_t launch_assemble_wave(int batch, int maxp, const float4 *peaks, const int *counts, const float4 *conns,
                                const float4 *aux, const int *conn_counts, const unsigned *status, pp_record *records,
                                hipStream_t stream);
hipError_t launch_limb_connect_hwc(const float *paf, int H, int W, int C, int maxp, int cap, int min_img_size,
                                   const float4 *peaks, const int *counts, float4 *conns, int *conn_counts,
                                   unsigned *status, hipStream_t stream);
// the drop-in process_paf's assembly, in the reference's order; peak ids are the .w bits of the peaks
hipError_t launch_assemble(int batch, int maxp, const float4 *peaks, const int *counts, const float4 *conns,
                           const int *conn_counts, const unsigned *status, int flag_first, pp_record *records,
                           hipStream_t stream);

// The Python-twin launchers take the context's test configuration (cfg; NULL = the INI defaults).  Each kernel's general
// instance is launched only when a value IT reads differs from the default; otherwise the instance with the literals runs.
size_t lds_bytes_limb_py(int elem, int h, int w, int maxp, int cap);
size_t lds_bytes_assemble_py(int maxp);
hipError_t launch_limb_connect_py(const void *net, int dtype, int batch, int n_samples, int h, int w, int flip, int maxp,
                                  int cap, int img_height, const int *img_height_dev, const float4 *peaks, const int *counts,
                                  void *conns, int *conn_counts, unsigned *status, const pp_test_cfg *cfg, hipStream_t stream);
hipError_t launch_assemble_py(int batch, int maxp, int explicit_ids, const float4 *peaks, const int *counts, const void *conns,
                              const int *conn_counts, const unsigned *status, int flag_first, pp_record *records,
                              double *persons_out, int *n_persons_out, const pp_test_cfg *cfg, hipStream_t stream);
hipError_t launch_limb_connect_py_hwc(const float *paf, int H, int W, int C, int maxp, int cap, int img_height,
                                      const float4 *peaks, const int *counts, void *conns, int *conn_counts, unsigned *status,
                                      const pp_test_cfg *cfg, hipStream_t stream);

hipError_t launch_resize_cubic(const float *src, long src_plane, int src_ld, int ch, int cw, void *dst, int acc, int C, int dh,
                               int dw, double scale_x, double scale_y, float n_div, hipStream_t stream);
hipError_t launch_flip_average_planar(const void *net, int dtype, int batch, int h, int w, int flip, float *out,
                                      hipStream_t stream);
hipError_t launch_accumulate_scales(int n_scales, const void *const *nets, int dtype, int batch, const int *hs, const int *ws,
                                    int flip, const int *pad_down, const int *pad_right, int img_h, int img_w, double *heat_acc,
                                    double *paf_acc, hipStream_t stream);
// ragged bucket: sizes / pads HOST (checks, grid, LDS caps), sizes_dev int[2][batch], pads_dev int[n_scales][2][batch]
hipError_t launch_accumulate_scales_ragged(int n_scales, const void *const *nets, int dtype, int batch, const int *hs, const int *ws,
                                           int flip, const int *sizes, const int *sizes_dev, const int *pads, const int *pads_dev,
                                           long slot_area, double *heat_acc, double *paf_acc, hipStream_t stream);
hipError_t launch_accumulate_scales_affine(int n_scales, const void *const *nets, int dtype, int batch, const int *hs, const int *ws,
                                           int flip, const int *pad_down, const int *pad_right, const double *const *m_inv,
                                           int img_h, int img_w, double *heat_acc, double *paf_acc, hipStream_t stream);
hipError_t launch_warp_affine_f32(const float *src, float *dst, long n, int h, int w, int channels, int hwc, const double *m_inv,
                                  hipStream_t stream);
hipError_t launch_fullres(int batch, int H, int W, float thre1, int maxp, int cap, int img_height, const double *heat_acc,
                          const double *paf_acc, unsigned char *mask_scratch, void *peaks64, int *counts, void *conns,
                          int *conn_counts, unsigned *status, pp_record *records, const pp_test_cfg *cfg, hipStream_t stream,
                          const int *sizes_dev = nullptr, long slot_area = 0);

}  // namespace pp
#endif
