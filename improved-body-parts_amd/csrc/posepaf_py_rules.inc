// posepaf_py_rules.inc -- the kernels of the Python-rule paths, compiled TWICE by posepaf_kernels.hip:
//   without PP_PY_CFG: the instances with the INI defaults as literals (0.1, 20, 0.8, 16, 0.7, radius 2, no remove_recon) under
//     their plain names.  Their token stream is the one they had before the run-time configuration existed, so they compile to
//     the same instructions (tools/default_asm_diff.py); these are launched whenever the context holds the defaults.
//   with PP_PY_CFG: the general instances `<name>_cfg`, which take a PyCfg by value as their last argument.
// A body wrapped into a shared __device__ template was tried first: inlining it changed register allocation and scheduling of
// the default instances, which is why the text is shared at the preprocessor level instead.
#ifdef PP_PY_CFG
#define PP_PYK(name) name##_cfg
#define PP_PY_CFG_PARAM , const PyCfg cfg
#define PP_PY_CFG_REF , const PyCfg &cfg
#define PP_PY_CFG_ARG , cfg
#define PP_PY_SCORE_PAIR(smp, ...) score_pair_py_cfg(smp, cfg, __VA_ARGS__)
#define PP_PY_LEN_RATE cfg.len_rate
#define PP_PY_CONNECTION_TOLE cfg.connection_tole
#else
#define PP_PYK(name) name
#define PP_PY_CFG_PARAM
#define PP_PY_CFG_REF
#define PP_PY_CFG_ARG
#define PP_PY_SCORE_PAIR(smp, ...) score_pair_py(smp, __VA_ARGS__)
#define PP_PY_LEN_RATE 16.0
#define PP_PY_CONNECTION_TOLE 0.7
#endif

// pafprocess-free Python rules for one limb: scoring, stable ranking, greedy pick, ordered output
template <typename Sampler>
__device__ void PP_PYK(connect_limb_py)(const Sampler &smp, const LimbLdsPy &L, int nA, int nB, int cap, int maxp, int ih,
                                double4 *__restrict__ conn_out, int *__restrict__ cc, unsigned *__restrict__ status_word PP_PY_CFG_REF) {
    __shared__ int s_wcnt[2][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- scoring + ordered compaction (generation order: src outer, dst inner)
    const int npairs = nA * nB;
    int ncand = 0, buf = 0;
    for (int base = 0; base < npairs; base += kThreads, buf ^= 1) {
        const int p = base + threadIdx.x;
        bool ok = false;
        double sc = 0, ov = 0, ln = 0;
        int ia = 0, ib = 0;
        if (p < npairs) {
            ia = p / nB;
            ib = p - ia * nB;
            ok = PP_PY_SCORE_PAIR(smp, L.ax[ia], L.ay[ia], L.as[ia], L.bx[ib], L.by[ib], L.bs[ib], ih, &sc, &ov, &ln);
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_wcnt[buf][wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            const int c = s_wcnt[buf][k];
            if (k < wave) before += c;
            all += c;
        }
        if (ok) {
            const int pos = ncand + before + __popcll(m & lanemask_lt());
            if (pos < cap) {
                L.key[pos] = ov;
                L.c_score[pos] = sc;
                L.c_len[pos] = ln;
                L.c_idx[pos] = (unsigned)ia | ((unsigned)ib << 16);
            }
        }
        ncand += all;
    }
    unsigned st = 0;
    if (ncand > cap) {
        st |= PP_ST_CAND_OVERFLOW;
        ncand = cap;
    }
    const int n = ncand;
    __syncthreads();
    // ---- sorted(reverse=True) is stable: equal keys keep generation order (:391)
    for (int t = threadIdx.x; t < n; t += kThreads) {
        const double kt = L.key[t];
        int r = 0;
        for (int j = 0; j < n; j++) {
            const double kj = L.key[j];
            r += (kj > kt) || (kj == kt && j < t);
        }
        L.rank[t] = r;
        L.state[t] = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += kThreads) L.order[L.rank[t]] = t;
    __syncthreads();
    // ---- greedy pick (:393-407) as repeated acceptance of locally dominant candidates (see connect_limb)
    for (int pass = 0; pass <= n; pass++) {  // every pass accepts at least the best live candidate: <= n passes
        for (int i = threadIdx.x; i < maxp; i += kThreads) {
            L.minA[i] = 0x7fffffff;
            L.minB[i] = 0x7fffffff;
        }
        __syncthreads();
        bool live = false;
        for (int t = threadIdx.x; t < n; t += kThreads) {
            if (L.state[t] == 0) {
                const unsigned idx = L.c_idx[t];
                const int ia = (int)(idx & 0xffffu), ib = (int)(idx >> 16);
                if (L.usedA[ia] || L.usedB[ib]) {
                    L.state[t] = 2;
                } else {
                    atomicMin(&L.minA[ia], L.rank[t]);
                    atomicMin(&L.minB[ib], L.rank[t]);
                    live = true;
                }
            }
        }
        if (!__syncthreads_or(live)) break;
        for (int t = threadIdx.x; t < n; t += kThreads) {
            if (L.state[t] == 0) {
                const unsigned idx = L.c_idx[t];
                const int ia = (int)(idx & 0xffffu), ib = (int)(idx >> 16);
                const int r = L.rank[t];
                if (L.minA[ia] == r && L.minB[ib] == r) {
                    L.state[t] = 1;
                    L.usedA[ia] = 1;
                    L.usedB[ib] = 1;
                }
            }
        }
        __syncthreads();
    }
    int ncn = 0;
    for (int base = 0; base < n; base += kThreads, buf ^= 1) {
        const int r = base + threadIdx.x;
        bool acc = false;
        int t = 0;
        if (r < n) {
            t = L.order[r];
            acc = L.state[t] == 1;
        }
        const unsigned long long m = __ballot(acc);
        if (lane == 0) s_wcnt[buf][wave] = __popcll(m);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            const int c = s_wcnt[buf][k];
            if (k < wave) before += c;
            all += c;
        }
        if (acc) {
            const unsigned idx = L.c_idx[t];
            conn_out[ncn + before + __popcll(m & lanemask_lt())] =
                make_double4((double)(idx & 0xffffu), (double)(idx >> 16), L.c_score[t], L.c_len[t]);
        }
        ncn += all;
    }
    if (threadIdx.x == 0) {
        *cc = ncn;
        *status_word = st;
    }
}

// LDS (dynamic): [map h*w T][cubic 16 f32][LimbLdsPy]
template <typename T>
__global__ __launch_bounds__(kThreads) void PP_PYK(k_limb_connect_py)(const T *__restrict__ net, int n_samples, int h, int w,
                                                              int flip, int maxp, int cap, int img_height,
                                                              const int *__restrict__ img_height_dev,
                                                              const float4 *__restrict__ peaks,
                                                              const int *__restrict__ counts, double4 *__restrict__ conns,
                                                              int *__restrict__ conn_counts,
                                                              unsigned *__restrict__ status PP_PY_CFG_PARAM) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int limb = blockIdx.x, img = blockIdx.y;
    const int pa = d_limb_pairs[limb][0], pb = d_limb_pairs[limb][1];
    int nA = counts[img * PP_NUM_PART + pa], nB = counts[img * PP_NUM_PART + pb];
    nA = nA < maxp ? nA : maxp;
    nB = nB < maxp ? nB : maxp;
    int *cc = conn_counts + img * PP_NUM_LIMB + limb;
    if (nA == 0 || nB == 0) {
        if (threadIdx.x == 0) {
            *cc = 0;
            status[img * kFlagWords + PP_NUM_PART + limb] = 0u;
        }
        return;
    }
    const int npix = h * w;
    size_t off = 0;
    T *smap = reinterpret_cast<T *>(lds_raw);
    off += (sizeof(T) * (size_t)npix + 15) & ~(size_t)15;
    float *s_cub = reinterpret_cast<float *>(lds_raw + off);
    off += 64;
    LimbLdsPy L = carve_limb_lds_py(lds_raw + off, maxp, cap);
    if (threadIdx.x < 16) s_cub[threadIdx.x] = d_cubic4[threadIdx.x >> 2][threadIdx.x & 3];
    const float4 *pka = peaks + ((size_t)img * PP_NUM_PART + pa) * maxp;
    const float4 *pkb = peaks + ((size_t)img * PP_NUM_PART + pb) * maxp;
    for (int i = threadIdx.x; i < nA; i += kThreads) {
        const float4 p = pka[i];
        L.ax[i] = p.x;
        L.ay[i] = p.y;
        L.as[i] = p.z;
    }
    for (int i = threadIdx.x; i < nB; i += kThreads) {
        const float4 p = pkb[i];
        L.bx[i] = p.x;
        L.by[i] = p.y;
        L.bs[i] = p.z;
    }
    for (int i = threadIdx.x; i < maxp; i += kThreads) {
        L.usedA[i] = 0;
        L.usedB[i] = 0;
    }
    const size_t plane = (size_t)npix;
    const T *o0 = net + ((size_t)img * n_samples * PP_NUM_CH + limb) * plane;
    const T *o1 = net + (((size_t)img * n_samples + 1) * PP_NUM_CH + d_flip_paf_ord[limb]) * plane;
    load_channel(smap, o0, o1, h, w, flip != 0);
    __syncthreads();
    LdsBicubicSampler<T> smp{smap, s_cub, h, w, w};
    const int ih = img_height_dev ? img_height_dev[img] : img_height;

    PP_PYK(connect_limb_py)(smp, L, nA, nB, cap, maxp, ih, conns + ((size_t)img * PP_NUM_LIMB + limb) * maxp, cc,
                            status + img * kFlagWords + PP_NUM_PART + limb PP_PY_CFG_ARG);
}

// Host-array form (utils.parse_skeletons.find_connections): the caller's up-sampled (H, W, C) map in global memory
__global__ __launch_bounds__(kThreads) void PP_PYK(k_limb_connect_py_hwc)(const float *__restrict__ paf, int H, int W, int C, int maxp,
                                                                  int cap, int img_height, const float4 *__restrict__ peaks,
                                                                  const int *__restrict__ counts, double4 *__restrict__ conns,
                                                                  int *__restrict__ conn_counts, unsigned *__restrict__ status PP_PY_CFG_PARAM) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int limb = blockIdx.x;
    const int pa = d_limb_pairs[limb][0], pb = d_limb_pairs[limb][1];
    int nA = counts[pa], nB = counts[pb];
    nA = nA < maxp ? nA : maxp;
    nB = nB < maxp ? nB : maxp;
    int *cc = conn_counts + limb;
    if (nA == 0 || nB == 0 || limb >= C) {
        if (threadIdx.x == 0) {
            *cc = 0;
            status[PP_NUM_PART + limb] = 0u;
        }
        return;
    }
    LimbLdsPy L = carve_limb_lds_py(lds_raw, maxp, cap);
    const float4 *pka = peaks + (size_t)pa * maxp;
    const float4 *pkb = peaks + (size_t)pb * maxp;
    for (int i = threadIdx.x; i < nA; i += kThreads) {
        const float4 p = pka[i];
        L.ax[i] = p.x;
        L.ay[i] = p.y;
        L.as[i] = p.z;
    }
    for (int i = threadIdx.x; i < nB; i += kThreads) {
        const float4 p = pkb[i];
        L.bx[i] = p.x;
        L.by[i] = p.y;
        L.bs[i] = p.z;
    }
    for (int i = threadIdx.x; i < maxp; i += kThreads) {
        L.usedA[i] = 0;
        L.usedB[i] = 0;
    }
    __syncthreads();
    GlobalHwcSampler smp{paf, H, W, C, limb};
    PP_PYK(connect_limb_py)(smp, L, nA, nB, cap, maxp, img_height, conns + (size_t)limb * maxp, cc,
                            status + PP_NUM_PART + limb PP_PY_CFG_ARG);
}

// find_humans, one wave per image, float64 person table in LDS: [s][k] = {id, score}; k = 18: {total, -1}; 19: {count, len}
#ifndef PP_PY_CFG
constexpr int kMaxSkelPy = 128;
__host__ __device__ inline size_t assemble_py_lds_bytes(int maxp) {
    return (size_t)kMaxSkelPy * kSkelStride * 16 + (size_t)PP_NUM_PART * maxp * 16 + (size_t)PP_NUM_LIMB * maxp * 32;
}
#endif

// PK = float4: refactored path (integer-valued coordinates, int x / y in the record); PK = double4: original path
// (fractional coordinates: the record's x / y fields then hold FLOAT bit patterns and PP_ST_FLOAT_COORDS is set).
template <typename PK>
__global__ __launch_bounds__(64) void PP_PYK(k_assemble_py)(int maxp, int explicit_ids, const PK *__restrict__ peaks,
                                                    const int *__restrict__ counts, const double4 *__restrict__ conns,
                                                    const int *__restrict__ conn_counts, const unsigned *__restrict__ status,
                                                    int flag_first, pp_record *__restrict__ records,
                                                    double *__restrict__ persons_out,
                                                    int *__restrict__ n_persons_out PP_PY_CFG_PARAM) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int img = blockIdx.x, lane = threadIdx.x;
    const int ntab = PP_NUM_PART * maxp;
    double *pid = reinterpret_cast<double *>(lds_raw);                 // [kMaxSkelPy][21]
    double *psc = pid + kMaxSkelPy * kSkelStride;
    double4 *s_conn = reinterpret_cast<double4 *>(psc + kMaxSkelPy * kSkelStride);  // {src_id, dst_id, score, len}
    float *line_x = reinterpret_cast<float *>(s_conn + PP_NUM_LIMB * maxp);
    float *line_y = line_x + ntab;
    float *line_s = line_y + ntab;
    constexpr bool kFloatCoords = sizeof(PK) == sizeof(double4);
    __shared__ int s_off[PP_NUM_PART + 1];
    __shared__ int s_cnt[PP_NUM_PART];
    __shared__ int s_coff[PP_NUM_LIMB + 1];
    __shared__ int s_merge;

    const int *cnt_g = counts + img * PP_NUM_PART;
    const PK *pk_g = peaks + (size_t)img * PP_NUM_PART * maxp;
    if (lane == 0) {
        int run = 0;
        for (int k = 0; k < PP_NUM_PART; k++) {
            int c = cnt_g[k];
            c = c < maxp ? c : maxp;
            s_cnt[k] = c;
            s_off[k] = run;
            run += c;
        }
        s_off[PP_NUM_PART] = run;
        run = 0;
        for (int l = 0; l < PP_NUM_LIMB; l++) {
            s_coff[l] = run;
            int c = conn_counts[img * PP_NUM_LIMB + l];
            run += c < maxp ? c : maxp;
        }
        s_coff[PP_NUM_LIMB] = run;
    }
    __syncthreads();
    const int n_peaks = s_off[PP_NUM_PART];
    for (int part = 0; part < PP_NUM_PART; part++) {  // joint_candidates: rows flattened in part order (:423)
        const int c = s_cnt[part], o = s_off[part];
        for (int r = lane; r < c; r += 64) {
            const PK p = pk_g[(size_t)part * maxp + r];
            line_x[o + r] = (float)p.x;
            line_y[o + r] = (float)p.y;
            line_s[o + r] = (float)p.z;
        }
    }
    for (int limb = 0; limb < PP_NUM_LIMB; limb++) {
        const int c = s_coff[limb + 1] - s_coff[limb], o = s_coff[limb];
        const int part1 = d_limb_pairs[limb][0], part2 = d_limb_pairs[limb][1];
        const double4 *cn_g = conns + ((size_t)img * PP_NUM_LIMB + limb) * maxp;
        for (int ci = lane; ci < c; ci += 64) {
            double4 cn = cn_g[ci];
            if (!explicit_ids) {  // peak id == position in the part-ordered joint list
                cn.x = (double)(s_off[part1] + (int)cn.x);
                cn.y = (double)(s_off[part2] + (int)cn.y);
            }
            s_conn[o + ci] = cn;
        }
    }
    __syncthreads();

    int np = 0;  // uniform
    unsigned st = 0;
    for (int limb = 0; limb < PP_NUM_LIMB; limb++) {
        const int part1 = d_limb_pairs[limb][0], part2 = d_limb_pairs[limb][1];
        for (int ci = s_coff[limb]; ci < s_coff[limb + 1]; ci++) {
            const double4 cn = s_conn[ci];
            const double src_id = cn.x, dst_id = cn.y, score = cn.z, limb_len = cn.w;
            int num_found = 0, idx1 = 0, idx2 = 0;
            for (int base = 0; base < np; base += 64) {  // :440-450; matches beyond the second are ignored
                const int s = base + lane;
                bool hit = false;
                if (s < np) hit = (pid[s * kSkelStride + part1] == src_id) || (pid[s * kSkelStride + part2] == dst_id);
                unsigned long long m = __ballot(hit);
                if (m) {
                    if (num_found == 0) {
                        idx1 = base + __ffsll((long long)m) - 1;
                        const unsigned long long m2 = m & (m - 1);
                        if (m2) idx2 = base + __ffsll((long long)m2) - 1;
                    } else if (num_found == 1) {
                        idx2 = base + __ffsll((long long)m) - 1;
                    }
                    num_found += __popcll(m);
                }
            }
            if (num_found > 2) num_found = 2;
            const int isrc = (int)src_id, idst = (int)dst_id;  // joint_candidates[int(id), 2]: indexed BY ID (:474, :589)
            const double ps_src = (isrc >= 0 && isrc < n_peaks) ? (double)line_s[isrc] : 0.0;
            const double ps_dst = (idst >= 0 && idst < n_peaks) ? (double)line_s[idst] : 0.0;
            if (num_found == 1) {  // :452-487
                if (lane == 0) {
                    double *i1 = pid + idx1 * kSkelStride, *f1 = psc + idx1 * kSkelStride;
                    const double dpk = i1[part2], dsc = f1[part2], plen = f1[19];
                    const bool len_ok = __dmul_rn(plen, PP_PY_LEN_RATE) > limb_len;
                    if ((int)dpk == -1 && len_ok) {
                        i1[part2] = dst_id;
                        f1[part2] = score;
                        i1[19] += 1.0;
                        f1[19] = limb_len > plen ? limb_len : plen;
                        i1[18] = __dadd_rn(i1[18], __dadd_rn(ps_dst, score));
                    } else if (((int)dpk != (int)dst_id && dsc <= score && len_ok) || ((int)dpk == (int)dst_id && dsc <= score)) {
                        // the OLD peak's score and the OLD limb score are subtracted first (:477-480)
                        const int old = (int)dpk;
                        const double old_ps = (old >= 0 && old < n_peaks) ? (double)line_s[old] : 0.0;
                        i1[18] = __dadd_rn(i1[18], -__dadd_rn(old_ps, dsc));
                        i1[part2] = dst_id;
                        f1[part2] = score;
                        f1[19] = limb_len > plen ? limb_len : plen;
                        i1[18] = __dadd_rn(i1[18], __dadd_rn(ps_dst, score));
                    }
                }
                __syncthreads();
            } else if (num_found == 2) {  // :489-560
                if (lane == 0) {
                    double *i1 = pid + idx1 * kSkelStride, *f1 = psc + idx1 * kSkelStride;
                    double *i2 = pid + idx2 * kSkelStride, *f2 = psc + idx2 * kSkelStride;
                    const double plen = f1[19];
                    bool shared = false, have1 = false, have2 = false;
                    double min1 = 0, min2 = 0;
                    for (int k = 0; k < PP_NUM_PART; k++) {
                        const bool m1 = i1[k] >= 0, m2 = i2[k] >= 0;  // :502-503
                        if (m1 && m2) shared = true;
                        if (m1 && (!have1 || f1[k] < min1)) { min1 = f1[k]; have1 = true; }
                        if (m2 && (!have2 || f2[k] < min2)) { min2 = f2[k]; have2 = true; }
                    }
                    int merge = 0;
                    if (!shared) {
                        const double mt = min1 < min2 ? min1 : min2;
                        if (score >= __dmul_rn(PP_PY_CONNECTION_TOLE, mt) && limb_len < __dmul_rn(plen, PP_PY_LEN_RATE)) {  // :511-512 AND
                            for (int k = 0; k < PP_NUM_PART; k++) {  // np.maximum on (18, 2), :516
                                if (i2[k] > i1[k]) i1[k] = i2[k];
                                if (f2[k] > f1[k]) f1[k] = f2[k];
                            }
                            i1[19] += i2[19];
                            f1[19] = limb_len > plen ? limb_len : plen;
                            i1[18] = __dadd_rn(i1[18], __dadd_rn(i2[18], score));
                            merge = 1;
                        }
#ifdef PP_PY_CFG
                    } else if (cfg.remove_recon > 0) {  // a joint shared by two people, :526-564 as written
                        // `id in ids` / np.where(ids == id) over the 18 part slots; int(...) of anything but exactly one match
                        // raises in the reference, as does the assert conn1_idx != conn2_idx: nothing changes, flag set
                        int n_src1 = 0, k_src1 = 0, n_dst1 = 0, k_dst1 = 0, n_src2 = 0, k_src2 = 0, n_dst2 = 0, k_dst2 = 0;
                        for (int k = 0; k < PP_NUM_PART; k++) {
                            if (i1[k] == src_id) { n_src1++; k_src1 = k; }
                            if (i1[k] == dst_id) { n_dst1++; k_dst1 = k; }
                            if (i2[k] == src_id) { n_src2++; k_src2 = k; }
                            if (i2[k] == dst_id) { n_dst2++; k_dst2 = k; }
                        }
                        const bool src_in_1 = n_src1 > 0;                                     // :529
                        const int n1 = src_in_1 ? n_src1 : n_dst1, n2 = src_in_1 ? n_dst2 : n_src2;
                        const int conn1 = src_in_1 ? k_src1 : k_dst1, conn2 = src_in_1 ? k_dst2 : k_src2;
                        if (n1 != 1 || n2 != 1 || conn1 == conn2) {
                            st |= PP_ST_RECON_UNDEFINED;
                        } else if (score >= f1[conn1] && score >= f2[conn2]) {                // :540-541
                            const bool low_is_2 = f1[conn1] > f2[conn2];                      // :545-552
                            double *il = low_is_2 ? i2 : i1, *fl = low_is_2 ? f2 : f1;
                            const int del = low_is_2 ? conn2 : conn1;
                            const int old = (int)il[del];
                            const double old_ps = (old >= 0 && old < n_peaks) ? (double)line_s[old] : 0.0;
                            il[18] = __dadd_rn(il[18], -__dadd_rn(old_ps, fl[del]));          // :556-558
                            il[del] = -1.0;
                            fl[del] = -1.0;
                            il[19] -= 1.0;
                        }
#endif
                    }
                    s_merge = merge;
                }
                __syncthreads();
                if (s_merge) {  // np.delete(person2)
                    for (int s = idx2; s < np - 1; s++) {
                        if (lane < 20) {
                            pid[s * kSkelStride + lane] = pid[(s + 1) * kSkelStride + lane];
                            psc[s * kSkelStride + lane] = psc[(s + 1) * kSkelStride + lane];
                        }
                    }
                    np--;
                }
                __syncthreads();
            } else {  // new person, :583-596
                if (np < kMaxSkelPy) {
                    if (lane < 20) {
                        double idv = -1.0, scv = -1.0;
                        if (lane == part1) { idv = src_id; scv = score; }
                        if (lane == part2) { idv = dst_id; scv = score; }
                        if (lane == 19) { idv = 2.0; scv = limb_len; }
                        if (lane == 18) idv = __dadd_rn(__dadd_rn(ps_src, ps_dst), score);
                        pid[np * kSkelStride + lane] = idv;
                        psc[np * kSkelStride + lane] = scv;
                    }
                    np++;
                } else {
                    st |= PP_ST_SKEL_OVERFLOW;
                }
                __syncthreads();
            }
        }
    }
    // ---- prune (:599-603) and records (evaluate.py:132-156: x, y, score from joint_candidates; score = total / count)
    pp_record *rec = records + img;
    int n_out = 0;
    for (int base = 0; base < np; base += 64) {
        const int s = base + lane;
        bool keep = false;
        if (s < np) {
            const double count = pid[s * kSkelStride + 19], total = pid[s * kSkelStride + 18];
            keep = !(count < 2.0 || total / count < 0.45);
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int r = n_out + __popcll(m & lanemask_lt());
            if (r < PP_MAX_HUMANS) {
                pp_human *hm = rec->humans + r;
                for (int kp = 0; kp < PP_NUM_PART; kp++) {
                    const int id = (int)pid[s * kSkelStride + kp];
                    hm->peak_id[kp] = id;
                    const bool ok = id >= 0 && id < n_peaks;
                    const float fx = ok ? line_x[id] : 0.0f, fy = ok ? line_y[id] : 0.0f;
                    hm->x[kp] = kFloatCoords ? __float_as_int(fx) : (int)fx;
                    hm->y[kp] = kFloatCoords ? __float_as_int(fy) : (int)fy;
                    hm->part_score[kp] = ok ? line_s[id] : 0.0f;
                }
                hm->score = (float)(pid[s * kSkelStride + 18] / pid[s * kSkelStride + 19]);
                hm->n_parts = (int)pid[s * kSkelStride + 19];
            }
            if (persons_out) {  // raw person_to_joint_assoc rows (20, 2) float64
                double *row = persons_out + (size_t)r * 40;
                for (int k = 0; k < 20; k++) {
                    row[2 * k] = pid[s * kSkelStride + k];
                    row[2 * k + 1] = psc[s * kSkelStride + k];
                }
            }
        }
        n_out += __popcll(m);
    }
    if (lane == 0 && n_persons_out) *n_persons_out = n_out;
    const unsigned fl = or_flags(status, img, flag_first, lane);
    if (lane == 0) {
        if (n_out > PP_MAX_HUMANS) {
            st |= PP_ST_HUMAN_OVERFLOW;
            n_out = PP_MAX_HUMANS;
        }
        rec->n_humans = n_out;
        rec->n_peaks = n_peaks;
        rec->n_connections = s_coff[PP_NUM_LIMB];
        rec->status = fl | st | (kFloatCoords ? PP_ST_FLOAT_COORDS : 0u);
    }
}

// find_peaks at image resolution: one workgroup per (part, image).  The float64 accumulator is cast to float32 on read
// (:290); 3x3 / >= thre NMS (reflect padding == ignore out-of-map neighbours); np.nonzero order via per-thread contiguous
// pixel ranges + block scan; refine_centroid per peak.  peaks: double4 (x, y, score, id-unused).
__global__ __launch_bounds__(kThreads) void PP_PYK(k_fullres_peaks)(const double *__restrict__ heat_acc, int H, int W, float thre,
                                                            int maxp, unsigned char *__restrict__ mask_scratch,
                                                            double4 *__restrict__ peaks, int *__restrict__ counts,
                                                            unsigned *__restrict__ status, const int *__restrict__ sizes,
                                                            long slot_area PP_PY_CFG_PARAM) {
    __shared__ int s_wsum[kWaves];
    __shared__ int s_pk[PP_MAX_PEAKS_PER_PART_LIMIT];
    const int part = blockIdx.x, img = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (sizes) {  // ragged bucket: this image's own extent, its planes dense at the head of slots of slot_area elements
        H = sizes[img];
        W = sizes[gridDim.y + img];
    }
    const long npix = (long)H * W;
    const long plane = sizes ? slot_area : npix;
    const double *M = heat_acc + ((long)img * PP_NUM_HEAT + part) * plane;
    unsigned char *mask = mask_scratch + ((long)img * PP_NUM_PART + part) * plane;
    auto val = [&](long i) -> float { return (float)M[i]; };
    for (long i = threadIdx.x; i < npix; i += kThreads) {
        const float v = val(i);
        unsigned char pk = 0;
        if (v >= thre) {
            const int y = (int)(i / W), x = (int)(i - (long)y * W);
            pk = 1;
            for (int dy = -1; dy <= 1 && pk; dy++) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -1; dx <= 1; dx++) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= W) continue;
                    if (val((long)yy * W + xx) > v) {
                        pk = 0;
                        break;
                    }
                }
            }
        }
        mask[i] = pk;
    }
    __syncthreads();  // same workgroup: its global writes are visible to it after the barrier
    const long ppt = (npix + kThreads - 1) / kThreads;
    const long b0 = (long)threadIdx.x * ppt;
    int cnt = 0;
    for (long q = b0; q < b0 + ppt && q < npix; q++) cnt += mask[q];
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(incl, d);
        if (lane >= d) incl += n;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int rank = incl - cnt;
    for (int q = 0; q < wave; q++) rank += s_wsum[q];
    int total = 0;
    for (int q = 0; q < kWaves; q++) total += s_wsum[q];
    for (long q = b0; q < b0 + ppt && q < npix && rank < maxp; q++)
        if (mask[q]) s_pk[rank++] = (int)q;
    __syncthreads();
    const int kept = total < maxp ? total : maxp;
    double4 *out = peaks + ((long)img * PP_NUM_PART + part) * maxp;
    for (int p = wave; p < kept; p += kWaves) {  // refine_centroid, radius 2 (utils/util.py:188-213)
        const int i = s_pk[p];
        const int py = i / W, px = i - py * W;
        double ox, oy, sc;
#ifdef PP_PY_CFG   // radius as a value, 0..7: a (2r+1)^2 box is at most 225 values, up to four per lane of the wave
        {
            const int R = cfg.offset_radius, side = 2 * R + 1, nbox = side * side;
            if (py - R < 0 || py + R + 1 > H || px - R < 0 || px + R + 1 > W) {  // utils/util.py:203-204
                ox = (double)px;
                oy = (double)py;
                sc = (double)val(i);
            } else {
                double sx = 0.0, sy = 0.0, sv = 0.0;
                for (int e = lane; e < nbox; e += 64) {
                    const int r = e / side, c = e - r * side;
                    const double v = (double)val((long)(py - R + r) * W + (px - R + c));
                    sx += v * (double)(r - R);  // x_grid varies along rows (np.mgrid): restated as written
                    sy += v * (double)(c - R);
                    sv += v;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    sx += __shfl_xor(sx, d);
                    sy += __shfl_xor(sy, d);
                    sv += __shfl_xor(sv, d);
                }
                ox = (double)px + sx / sv;
                oy = (double)py + sy / sv;
                sc = sv / (double)nbox;
            }
        }
#else
        if (py - 2 < 0 || py + 3 > H || px - 2 < 0 || px + 3 > W) {
            ox = (double)px;
            oy = (double)py;
            sc = (double)val(i);
        } else {
            double sx = 0.0, sy = 0.0, sv = 0.0;
            if (lane < 25) {
                const int r = lane / 5, c = lane - r * 5;
                const double v = (double)val((long)(py - 2 + r) * W + (px - 2 + c));
                sx = v * (double)(r - 2);  // x_grid varies along rows (np.mgrid): restated as written
                sy = v * (double)(c - 2);
                sv = v;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sx += __shfl_xor(sx, d);
                sy += __shfl_xor(sy, d);
                sv += __shfl_xor(sv, d);
            }
            ox = (double)px + sx / sv;
            oy = (double)py + sy / sv;
            sc = sv / 25.0;
        }
#endif
        if (lane == 0) out[p] = make_double4(ox, oy, (double)(float)sc, 0.0);  // box.mean() is a float32 scalar
    }
    if (threadIdx.x == 0) {
        counts[img * PP_NUM_PART + part] = total;
        status[img * kFlagWords + part] = total > maxp ? PP_ST_PEAK_OVERFLOW : 0u;  // plain store, every launch
    }
}

#ifndef PP_PY_CFG
struct GlobalPlanarF64Sampler {  // predict's paf_avg, planar (30, H, W) float64
    const double *paf;
    int H, W;
    __device__ __forceinline__ double at(int X, int Y) const {
        X = clampi(X, 0, W - 1);
        Y = clampi(Y, 0, H - 1);
        return paf[(long)Y * W + X];
    }
};
#endif

__global__ __launch_bounds__(kThreads) void PP_PYK(k_limb_connect_py_fullres)(const double *__restrict__ paf_acc, int H, int W, int maxp,
                                                                      int cap, int img_height,
                                                                      const double4 *__restrict__ peaks,
                                                                      const int *__restrict__ counts, double4 *__restrict__ conns,
                                                                      int *__restrict__ conn_counts, unsigned *__restrict__ status,
                                                                      const int *__restrict__ sizes, long slot_area PP_PY_CFG_PARAM) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int limb = blockIdx.x, img = blockIdx.y;
    long plane = (long)H * W;
    if (sizes) {  // ragged bucket: the sampler clamps to this image's own extent; img_h of find_connections is its height
        H = sizes[img];
        W = sizes[gridDim.y + img];
        img_height = H;
        plane = slot_area;
    }
    const int pa = d_limb_pairs[limb][0], pb = d_limb_pairs[limb][1];
    int nA = counts[img * PP_NUM_PART + pa], nB = counts[img * PP_NUM_PART + pb];
    nA = nA < maxp ? nA : maxp;
    nB = nB < maxp ? nB : maxp;
    int *cc = conn_counts + img * PP_NUM_LIMB + limb;
    if (nA == 0 || nB == 0) {
        if (threadIdx.x == 0) {
            *cc = 0;
            status[img * kFlagWords + PP_NUM_PART + limb] = 0u;
        }
        return;
    }
    LimbLdsPy L = carve_limb_lds_py(lds_raw, maxp, cap);
    const double4 *pka = peaks + ((long)img * PP_NUM_PART + pa) * maxp;
    const double4 *pkb = peaks + ((long)img * PP_NUM_PART + pb) * maxp;
    for (int i = threadIdx.x; i < nA; i += kThreads) {
        const double4 p = pka[i];
        L.ax[i] = p.x;
        L.ay[i] = p.y;
        L.as[i] = p.z;
    }
    for (int i = threadIdx.x; i < nB; i += kThreads) {
        const double4 p = pkb[i];
        L.bx[i] = p.x;
        L.by[i] = p.y;
        L.bs[i] = p.z;
    }
    for (int i = threadIdx.x; i < maxp; i += kThreads) {
        L.usedA[i] = 0;
        L.usedB[i] = 0;
    }
    __syncthreads();
    GlobalPlanarF64Sampler smp{paf_acc + ((long)img * PP_NUM_LIMB + limb) * plane, H, W};
    PP_PYK(connect_limb_py)(smp, L, nA, nB, cap, maxp, img_height, conns + ((long)img * PP_NUM_LIMB + limb) * maxp, cc,
                            status + img * kFlagWords + PP_NUM_PART + limb PP_PY_CFG_ARG);
}


#undef PP_PYK
#undef PP_PY_CFG_PARAM
#undef PP_PY_CFG_REF
#undef PP_PY_CFG_ARG
#undef PP_PY_SCORE_PAIR
#undef PP_PY_LEN_RATE
#undef PP_PY_CONNECTION_TOLE
