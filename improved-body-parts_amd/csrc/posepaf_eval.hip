// posepaf_eval.hip -- the per-image half of the COCO keypoint evaluation on the device, straight from pp_record[b]:
//   pp_coco_rows_f32  records -> result rows, what coco.humans_from_record + coco.coco_results build one object at a time
//                     (reference evaluate.py:111-129, :182-209): per human with at least one part 17 x (x, y, 1) in COCO order,
//                     zeros for absent parts, then the human's score;
//   pp_oks_match      rows + packed ground truth -> stage A of posepaf/oks_eval.py evaluate_keypoints_ranges (match_image): the
//                     20 best detections in stable order, the OKS matrix, and the greedy matching at 10 thresholds x 3 area
//                     ranges, ONE WAVE PER IMAGE, one lane per (range, threshold) pair for the sequential part.
// The OKS argument is formed by compute_oks' IEEE operations one at a time in float64 (csrc/Makefile STRICT: no contraction):
//   e = (dx * dx + dy * dy) / var / (area + 2.220446049250313e-16) / 2,   oks = sum(exp(-e)) / count
// so only exp (the device library's, within an ulp) and the order of the sum (sequential here, pairwise in NumPy) can differ from
// the host: tests/test_gpu_ap_device.py bounds the matrix by 1e-13 and asks the flags to be exact on inputs whose OKS values keep
// a margin to every threshold.  Thresholds and area ranges are the host's own float64 values (np.linspace), passed by value.
// No atomics, no allocation, nothing shared between workgroups; every output word is stored plainly on every launch.
#include <hip/hip_runtime.h>

#include "../../include/posepaf.h"

namespace {

constexpr int ROW = PP_COCO_ROW;
constexpr int ROWS_THREADS = PP_MAX_HUMANS;      // one thread per human of the record
constexpr int MD = PP_AP_MAX_DETS, MG = PP_AP_MAX_GT, NT = PP_AP_THRESHOLDS, NR = PP_AP_RANGES;
static_assert(PP_MAX_HUMANS == 128 && MG == 128, "two ballots of 64 lanes cover a record / an image's ground truth");

// posepaf/skeleton.py ORDER_COCO (reference evaluate.py:40): COCO keypoint k is CMU part d_order_coco[k]
__device__ const signed char d_order_coco[17] = {0, 15, 14, 17, 16, 5, 2, 6, 3, 7, 4, 11, 8, 12, 9, 13, 10};

// (KPT_SIGMAS * 2) ** 2 of posepaf/oks_eval.py, KPT_SIGMAS = [.26, ...] / 10.0: the same three IEEE operations, folded by the compiler
#define PP_VAR(s) ((((s) / 10.0) * 2) * (((s) / 10.0) * 2))
__device__ const double d_var[17] = {PP_VAR(.26),  PP_VAR(.25),  PP_VAR(.25), PP_VAR(.35), PP_VAR(.35), PP_VAR(.79),
                                     PP_VAR(.79),  PP_VAR(.72),  PP_VAR(.72), PP_VAR(.62), PP_VAR(.62), PP_VAR(1.07),
                                     PP_VAR(1.07), PP_VAR(.87),  PP_VAR(.87), PP_VAR(.89), PP_VAR(.89)};
#undef PP_VAR

// np.rint(float32).astype(np.int32) of a PP_ST_FLOAT_COORDS coordinate: round half to even (saturated; NaN -> 0: NumPy's own
// result there is not defined)
__device__ __forceinline__ int coord_of(int raw, bool is_float) {
    if (!is_float) return raw;
    const float f = __int_as_float(raw);
    if (!(f == f)) return 0;
    const float r = rintf(f);
    if (r >= 2147483648.0f) return 2147483647;
    if (r <= -2147483648.0f) return -2147483647 - 1;
    return (int)r;
}

__global__ __launch_bounds__(ROWS_THREADS) void k_coco_rows(const pp_record *__restrict__ recs, float *__restrict__ rows,
                                                            int *__restrict__ counts) {
    __shared__ unsigned long long s_mask[2];
    __shared__ unsigned char s_list[PP_MAX_HUMANS];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const pp_record *rec = recs + b;
    const int nh = min(max(rec->n_humans, 0), PP_MAX_HUMANS);
    const bool is_float = (rec->status & PP_ST_FLOAT_COORDS) != 0;

    // ---- the humans with at least one part, in record order
    bool keep = false;
    if (tid < nh) {
        const pp_human *hm = rec->humans + tid;
        for (int p = 0; p < PP_NUM_PART; p++) keep = keep || hm->peak_id[p] >= 0;
    }
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) s_mask[tid >> 6] = m;
    __syncthreads();
    const int n0 = __popcll(s_mask[0]);
    const int n = n0 + __popcll(s_mask[1]);
    if (keep) {
        const unsigned long long below = m & ((1ull << (tid & 63)) - 1ull);
        s_list[(tid >= 64 ? n0 : 0) + __popcll(below)] = (unsigned char)tid;
    }
    __syncthreads();

    // ---- all 128 x 52 words of the image's slot, consecutive threads to consecutive words; zeros past the last human
    float *out = rows + b * (long)(PP_MAX_HUMANS * ROW);
    for (int e = tid; e < PP_MAX_HUMANS * ROW; e += ROWS_THREADS) {
        const int r = e / ROW, c = e - r * ROW;
        float v = 0.0f;
        if (r < n) {
            const pp_human *hm = rec->humans + s_list[r];
            if (c == ROW - 1) {
                v = hm->score;
            } else {
                const int k = c / 3, j = c - k * 3;
                const int part = d_order_coco[k];
                if (hm->peak_id[part] >= 0) v = j == 2 ? 1.0f : (float)coord_of(j == 0 ? hm->x[part] : hm->y[part], is_float);
            }
        }
        out[e] = v;
    }
    if (tid == 0) counts[b] = n;
}

struct MatchParams {
    double thr[NT];
    double rng[NR][2];
};

// compute_oks(dt, gt.keypoints, gt.area, gt.bbox) of posepaf/oks_eval.py; dt: one row (17 x (x, y, 1) float32)
__device__ double oks_of(const float *__restrict__ dt, const pp_gt_ann *__restrict__ g) {
    int k1 = 0;
    for (int k = 0; k < 17; k++) k1 += g->keypoints[k][2] > 0.0 ? 1 : 0;
    const double area_eps = g->area + 2.220446049250313e-16;
    double sum = 0.0;
    if (k1 > 0) {
        for (int k = 0; k < 17; k++) {
            if (!(g->keypoints[k][2] > 0.0)) continue;
            const double dx = (double)dt[3 * k] - g->keypoints[k][0], dy = (double)dt[3 * k + 1] - g->keypoints[k][1];
            const double xx = dx * dx, yy = dy * dy;
            const double e = (xx + yy) / d_var[k] / area_eps / 2.0;
            sum += exp(-e);
        }
        return sum / (double)k1;
    }
    if (!g->has_bbox) return 0.0;
    // no labelled keypoint: distance to the doubled box
    const double w = g->bbox[2], h = g->bbox[3];
    const double x1 = g->bbox[0] + 2.0 * w, y1 = g->bbox[1] + 2.0 * h;
    const double x0 = g->bbox[0] - w, y0 = g->bbox[1] - h;
    for (int k = 0; k < 17; k++) {
        const double xd = (double)dt[3 * k], yd = (double)dt[3 * k + 1];
        const double dx = fmax(0.0, x0 - xd) + fmax(0.0, xd - x1), dy = fmax(0.0, y0 - yd) + fmax(0.0, yd - y1);
        const double xx = dx * dx, yy = dy * dy;
        const double e = (xx + yy) / d_var[k] / area_eps / 2.0;
        sum += exp(-e);
    }
    return sum / 17.0;
}

__global__ __launch_bounds__(64) void k_oks_match(const float *__restrict__ rows, const int *__restrict__ counts,
                                                  const pp_gt_ann *__restrict__ gt, const int *__restrict__ gt_off,
                                                  const int *__restrict__ slots, MatchParams P, int *__restrict__ order_out,
                                                  float *__restrict__ scores_out, signed char *__restrict__ match_out,
                                                  int *__restrict__ ndet_out, int *__restrict__ ngt_out, double *oks_out) {
    __shared__ double s_oks[MD * MG];             // 20 KB: [detection in score order][ground truth in annotation order]
    __shared__ double s_darea[MD];
    __shared__ double s_thr[NT], s_rng[NR][2];
    __shared__ float s_score[PP_MAX_HUMANS], s_key[PP_MAX_HUMANS];
    __shared__ int s_order[MD];
    __shared__ int s_nreal[NR];
    __shared__ unsigned char s_perm[NR][MG];      // per range: ground truths, the counted ones first, stable
    __shared__ unsigned char s_crowd[MG];

    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const int n = min(max(counts[b], 0), PP_MAX_HUMANS);
    const float *row = rows + b * (long)(PP_MAX_HUMANS * ROW);
    const int slot = slots ? slots[b] : (int)b;
    const int g0 = gt_off[slot];
    const int G = min(max(gt_off[slot + 1] - g0, 0), MG);
    const pp_gt_ann *anns = gt + g0;

    for (int i = lane; i < PP_MAX_HUMANS; i += 64) {
        const float s = i < n ? row[i * ROW + ROW - 1] : 0.0f;
        s_score[i] = s;
        s_key[i] = s == s ? s : -INFINITY;      // a NaN score has no place in Python's sort either: last, so that the ranks stay a permutation
    }
    if (lane < MD) s_order[lane] = -1;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NT; k++) s_thr[k] = P.thr[k];
#pragma unroll
        for (int k = 0; k < NR; k++) s_rng[k][0] = P.rng[k][0], s_rng[k][1] = P.rng[k][1];
    }
    __syncthreads();

    // ---- the 20 best detections by score, ties in row order: sorted(d, key=-score)[:20]
    for (int i = lane; i < n; i += 64) {
        const float s = s_key[i];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const float sj = s_key[j];
            rank += (sj > s || (sj == s && j < i)) ? 1 : 0;
        }
        if (rank < MD) s_order[rank] = i;
    }
    __syncthreads();
    const int D = min(n, MD);

    // ---- detection areas: the box of all 17 entries, missing parts' (0, 0) included
    if (lane < D) {
        const float *dt = row + s_order[lane] * ROW;
        float x0 = dt[0], x1 = dt[0], y0 = dt[1], y1 = dt[1];
        for (int k = 1; k < 17; k++) {
            x0 = fminf(x0, dt[3 * k]), x1 = fmaxf(x1, dt[3 * k]);
            y0 = fminf(y0, dt[3 * k + 1]), y1 = fmaxf(y1, dt[3 * k + 1]);
        }
        const double w = (double)x1 - (double)x0, h = (double)y1 - (double)y0;
        s_darea[lane] = w * h;
    }

    // ---- OKS matrix
    for (int e = lane; e < D * G; e += 64) {
        const int d = e / G, g = e - d * G;
        s_oks[d * MG + g] = oks_of(row + s_order[d] * ROW, anns + g);
    }

    // ---- per range: which ground truths count, and their order (counted first, stable)
    for (int r = 0; r < NR; r++) {
        const double lo = s_rng[r][0], hi = s_rng[r][1];
        bool real[2], ign[2];
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int g = lane + 64 * half;
            real[half] = ign[half] = false;
            if (g < G) {
                const pp_gt_ann *a = anns + g;
                const bool ig = a->iscrowd != 0 || a->num_keypoints == 0 || a->area < lo || a->area > hi;
                real[half] = !ig, ign[half] = ig;
                if (r == 0) s_crowd[g] = a->iscrowd != 0;
            }
        }
        const unsigned long long mr0 = __ballot(real[0]), mr1 = __ballot(real[1]);
        const unsigned long long mi0 = __ballot(ign[0]), mi1 = __ballot(ign[1]);
        const unsigned long long below = (1ull << lane) - 1ull;
        const int nr0 = __popcll(mr0), nreal = nr0 + __popcll(mr1), ni0 = __popcll(mi0);
        if (real[0]) s_perm[r][__popcll(mr0 & below)] = (unsigned char)lane;
        if (real[1]) s_perm[r][nr0 + __popcll(mr1 & below)] = (unsigned char)(lane + 64);
        if (ign[0]) s_perm[r][nreal + __popcll(mi0 & below)] = (unsigned char)lane;
        if (ign[1]) s_perm[r][nreal + ni0 + __popcll(mi1 & below)] = (unsigned char)(lane + 64);
        if (lane == 0) s_nreal[r] = nreal;
    }
    __syncthreads();

    // ---- greedy matching: lane t = range * 10 + threshold walks the detections in order (evaluate_keypoints' loop)
    if (lane < NR * NT) {
        const int r = lane / NT, ti = lane - r * NT;
        const double thr = s_thr[ti], lo = s_rng[r][0], hi = s_rng[r][1];
        const double cap = 1 - 1e-10;
        const double start = cap < thr ? cap : thr;          // min(thr, 1 - 1e-10)
        const int nreal = s_nreal[r];
        unsigned long long taken0 = 0, taken1 = 0;            // by position in the range's order
        signed char *mo = match_out + ((b * NR + r) * NT + ti) * MD;
        for (int i = 0; i < MD; i++) {
            signed char flag = 0;
            if (i < D) {
                double best = start;
                int bj = -1;
                for (int j = 0; j < G; j++) {
                    const int g = s_perm[r][j];
                    const bool tk = j < 64 ? (taken0 >> j) & 1ull : (taken1 >> (j - 64)) & 1ull;
                    if (tk && !s_crowd[g]) continue;           // a crowd region may absorb any number of detections
                    if (bj > -1 && bj < nreal && j >= nreal) break;
                    const double o = s_oks[i * MG + g];
                    if (o < best) continue;
                    best = o, bj = j;
                }
                if (bj >= 0) {
                    if (bj < 64) taken0 |= 1ull << bj; else taken1 |= 1ull << (bj - 64);
                    flag = bj >= nreal ? -1 : 1;
                } else {
                    const double da = s_darea[i];
                    flag = (da < lo || da > hi) ? -1 : 0;
                }
            }
            mo[i] = flag;
        }
    }

    // ---- the rest of the image's outputs
    if (lane < MD) {
        const int o = lane < D ? s_order[lane] : -1;
        order_out[b * MD + lane] = o;
        scores_out[b * MD + lane] = o >= 0 ? s_score[o] : 0.0f;
    }
    if (lane < NR) ngt_out[b * NR + lane] = s_nreal[lane];
    if (lane == 0) ndet_out[b] = D;
    if (oks_out) {
        double *oo = oks_out + b * (long)(MD * MG);
        for (int e = lane; e < MD * MG; e += 64) {
            const int d = e / MG, g = e - d * MG;
            oo[e] = (d < D && g < G) ? s_oks[e] : 0.0;
        }
    }
}
}  // namespace

extern "C" int pp_coco_rows_f32(const pp_record *records_dev, int batch, float *rows_dev, int *counts_dev, void *stream) {
    if (!records_dev || !rows_dev || !counts_dev || batch <= 0) return PP_ERR_BAD_ARG;
    hipLaunchKernelGGL(k_coco_rows, dim3((unsigned)batch), dim3(ROWS_THREADS), 0, static_cast<hipStream_t>(stream), records_dev,
                       rows_dev, counts_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}

extern "C" int pp_oks_match(const float *rows_dev, const int *counts_dev, int batch, const pp_gt_ann *gt_dev, const int *gt_offsets_dev,
                            const int *gt_offsets_host, int n_slots, const int *slots_dev, const int *slots_host,
                            const double *thresholds, const double *area_ranges, int *order_dev, float *scores_dev,
                            signed char *match_dev, int *n_det_dev, int *n_gt_dev, double *oks_dev, void *stream) {
    if (!rows_dev || !counts_dev || batch <= 0 || !gt_offsets_dev || !gt_offsets_host || n_slots <= 0 || !thresholds || !area_ranges ||
        !order_dev || !scores_dev || !match_dev || !n_det_dev || !n_gt_dev)
        return PP_ERR_BAD_ARG;
    if ((slots_dev == nullptr) != (slots_host == nullptr)) return PP_ERR_BAD_ARG;
    if (!slots_host && batch > n_slots) return PP_ERR_BAD_ARG;
    bool any_gt = false;
    for (int b = 0; b < batch; b++) {   // every image's ground truth must fit the kernel's LDS matrix: refused, never truncated
        const int s = slots_host ? slots_host[b] : b;
        if (s < 0 || s >= n_slots) return PP_ERR_BAD_ARG;
        const long cnt = (long)gt_offsets_host[s + 1] - (long)gt_offsets_host[s];
        if (cnt < 0 || gt_offsets_host[s] < 0) return PP_ERR_BAD_ARG;
        if (cnt > MG) return PP_ERR_TOO_LARGE;
        any_gt = any_gt || cnt > 0;
    }
    if (any_gt && !gt_dev) return PP_ERR_BAD_ARG;
    MatchParams P;
    for (int k = 0; k < NT; k++) P.thr[k] = thresholds[k];
    for (int k = 0; k < NR; k++) P.rng[k][0] = area_ranges[2 * k], P.rng[k][1] = area_ranges[2 * k + 1];
    hipLaunchKernelGGL(k_oks_match, dim3((unsigned)batch), dim3(64), 0, static_cast<hipStream_t>(stream), rows_dev, counts_dev, gt_dev,
                       gt_offsets_dev, slots_dev, P, order_dev, scores_dev, match_dev, n_det_dev, n_gt_dev, oks_dev);
    return hipGetLastError() == hipSuccess ? PP_OK : PP_ERR_HIP;
}
