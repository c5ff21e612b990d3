// posepaf_map_kernels.inc -- the text of K_A (k_heat_peaks) and K_B (k_limb_connect), included by posepaf_kernels.hip at the
// places where the two kernels stand (PP_INC_KA / PP_INC_KB select the part) and, with PP_MAPS_HBM defined, once more for
// the instances that leave the feature map in device memory (k_heat_peaks_hbm / k_limb_connect_hbm, DESIGN.md section 3).
// Without PP_MAPS_HBM the preprocessor hands the compiler the token stream the two kernels always had, so the instances that
// run on maps that fit LDS do not change (tools/default_asm_diff.py, DESIGN.md section 6); with it, only the places where the
// map's residency shows differ: where `smap` points (the plane of k_flip_average_maps' workspace ws[B][kWsChannels][ws_stride]
// instead of LDS), no load_channel, K_B's sampler (PP_LIMB_SAMPLER), and LDS of its own for K_A's image sorter.
#ifdef PP_INC_KA
#ifdef PP_MAPS_HBM
// Every global read of the map is in range by construction (a plane holds ws_stride >= h*w elements and starts on a 16-byte
// boundary):
//  - mask8's 16-byte vectors start at pixel i0 = 8v and are read whole only when i0 + 8 <= h*w; the ragged last vector takes the
//    per-pixel reads, each guarded by i0 + j < h*w;
//  - the rows above / below (load8 at i0 -/+ w, only when w % 8 == 0, so they stay 16-byte aligned) are guarded by y > 0 /
//    y < h - 1, the left / right / diagonal scalars by x0 > 0 / x0 + 8 < w and the same row guards; the per-pixel form for other
//    widths guards every neighbour at the map border;
//  - refinement: the centroid's 5 x 5 box is read only when it lies inside the map; the bicubic patch's taps are clamped to
//    the window [y_min, y_max] x [x_min, x_max], itself clamped to the map.
// LDS layout (dynamic): [cubic 16 f32][peak linear index i32 x maxp][peak-mask bytes x ceil(h*w/8)][image sorter: B i32]
#endif
template <typename T>
#ifndef PP_MAPS_HBM
__global__ __launch_bounds__(kThreads) void k_heat_peaks(const T *__restrict__ net, int n_samples, int h, int w,
                                                         int flip, int refine, int nms_mode, float thr, int maxp,
                                                         float4 *__restrict__ peaks, int *counts,
                                                         unsigned *__restrict__ status, int *order, int *arrive_all) {
#else
__global__ __launch_bounds__(kThreads) void k_heat_peaks_hbm(const T *__restrict__ ws, size_t ws_stride, int h, int w, int refine,
                                                             int nms_mode, float thr, int maxp, float4 *__restrict__ peaks,
                                                             int *counts, unsigned *__restrict__ status, int *order,
                                                             int *arrive_all) {
#endif
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int part = blockIdx.x, img = blockIdx.y;
    const int npix = h * w;
    size_t off = 0;
#ifndef PP_MAPS_HBM
    T *smap = reinterpret_cast<T *>(lds_raw);
    off += (sizeof(T) * (size_t)npix + 15) & ~(size_t)15;
#else
    const T *smap = ws + ((size_t)img * kWsChannels + PP_NUM_LIMB + part) * ws_stride;   // this part's plane of the workspace
#endif
    float *s_cub = reinterpret_cast<float *>(lds_raw + off);
    off += 64;
    int *s_pk = reinterpret_cast<int *>(lds_raw + off);
    off += (4 * (size_t)maxp + 15) & ~(size_t)15;
    unsigned char *s_m8 = lds_raw + off;  // one peak-mask byte per 8-pixel vector
    __shared__ int s_wsum[kWaves];
    __shared__ float s_hpass[kWaves][5 * 20];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) s_cub[threadIdx.x] = d_cubic4[threadIdx.x >> 2][threadIdx.x & 3];

#ifndef PP_MAPS_HBM
    const size_t plane = (size_t)npix;
    const T *o0 = net + ((size_t)img * n_samples * PP_NUM_CH + PP_NUM_LIMB + part) * plane;
    const T *o1 = net + (((size_t)img * n_samples + 1) * PP_NUM_CH + PP_NUM_LIMB + d_flip_heat_ord[part]) * plane;
#endif
    long long *stamps = d_stamps;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    stamp(stamps, wg, 0);
#ifndef PP_MAPS_HBM
    load_channel(smap, o0, o1, h, w, flip != 0);
#endif
    __syncthreads();
    stamp(stamps, wg, 1);

    // ---- A3: local maxima.  Each lane tests 8 consecutive row-major pixels per step (one 16-byte LDS read for
    // binary16 maps); only pixels above the threshold (a few per cent) go on to the neighbour reads.  Peak order must
    // be np.nonzero's (ascending linear index): per-(step, wave) counts -> block prefix -> lane prefix -> bit rank.
    const int nvec = (npix + 7) >> 3;
    const int nk = (nvec + kThreads - 1) / kThreads;  // steps of the run-time loops below; no bound on them (302 at 650 x 950)
    const bool rows_aligned = (w & 7) == 0;  // then an 8-pixel vector never straddles two rows
    auto mask8 = [&](int v) -> unsigned {
        const int i0 = v << 3;
        if (i0 >= npix) return 0u;
        float val[8];
        if (i0 + 8 <= npix) {
            load8(smap + i0, val);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) val[j] = i0 + j < npix ? ldsf(smap, i0 + j) : -INFINITY;
        }
        unsigned above = 0;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (nms_mode == 0 ? (val[j] > thr) : (val[j] >= thr)) above |= 1u << j;  // parse_skeletons.py:116 / util.py:184
        if (above == 0) return 0u;
        unsigned m = 0;
        if (rows_aligned) {
            // branch-free form: the rows above/below as two more 16-byte reads, the horizontal neighbours from the
            // vector itself plus one scalar on each side; out-of-map neighbours are -inf (never greater)
            const int y = i0 / w, x0 = i0 - y * w;
            float up[8], dn[8];
            if (y > 0) load8(smap + i0 - w, up);
            if (y < h - 1) load8(smap + i0 + w, dn);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (y == 0) up[j] = -INFINITY;
                if (y == h - 1) dn[j] = -INFINITY;
            }
            const float lft = x0 > 0 ? ldsf(smap, i0 - 1) : -INFINITY;
            const float rgt = x0 + 8 < w ? ldsf(smap, i0 + 8) : -INFINITY;
            float ul = -INFINITY, ur = -INFINITY, dl = -INFINITY, dr = -INFINITY;
            if (nms_mode != 0) {
                if (y > 0 && x0 > 0) ul = ldsf(smap, i0 - w - 1);
                if (y > 0 && x0 + 8 < w) ur = ldsf(smap, i0 - w + 8);
                if (y < h - 1 && x0 > 0) dl = ldsf(smap, i0 + w - 1);
                if (y < h - 1 && x0 + 8 < w) dr = ldsf(smap, i0 + w + 8);
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const float vj = val[j];
                bool pk = !(up[j] > vj) && !(dn[j] > vj);
                pk = pk && !((j > 0 ? val[j - 1] : lft) > vj) && !((j < 7 ? val[j + 1] : rgt) > vj);
                if (nms_mode != 0) {  // full 3x3 window (utils/util.py:181-184)
                    pk = pk && !((j > 0 ? up[j - 1] : ul) > vj) && !((j < 7 ? up[j + 1] : ur) > vj);
                    pk = pk && !((j > 0 ? dn[j - 1] : dl) > vj) && !((j < 7 ? dn[j + 1] : dr) > vj);
                }
                if (pk) m |= 1u << j;
            }
            return m & above;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (above & (1u << j)) {
                const float vj = val[j];
                const int i = i0 + j;
                const int y = i / w, x = i - y * w;
                bool pk = true;
                if (y > 0 && ldsf(smap, i - w) > vj) pk = false;
                if (y < h - 1 && ldsf(smap, i + w) > vj) pk = false;
                if (x > 0 && ldsf(smap, i - 1) > vj) pk = false;
                if (x < w - 1 && ldsf(smap, i + 1) > vj) pk = false;
                if (nms_mode != 0) {
                    if (y > 0 && x > 0 && ldsf(smap, i - w - 1) > vj) pk = false;
                    if (y > 0 && x < w - 1 && ldsf(smap, i - w + 1) > vj) pk = false;
                    if (y < h - 1 && x > 0 && ldsf(smap, i + w - 1) > vj) pk = false;
                    if (y < h - 1 && x < w - 1 && ldsf(smap, i + w + 1) > vj) pk = false;
                }
                if (pk) m |= 1u << j;
            }
        }
        return m;
    };
    for (int k = 0; k < nk; k++) {
        const int v = k * kThreads + threadIdx.x;
        const unsigned m8 = mask8(v);
        if (v < nvec) s_m8[v] = (unsigned char)m8;
    }
    __syncthreads();
    // Thread t now owns mask bytes [t*bpt, (t+1)*bpt), i.e. a CONTIGUOUS pixel range, so peak order (np.nonzero:
    // ascending linear index) is thread order: one block scan of the per-thread counts gives every peak's rank.
    const int bpt = nk;  // == ceil(nvec / kThreads)
    const int b0 = threadIdx.x * bpt;
    int cnt = 0;
    unsigned long long word = 0;
    const bool one_word = bpt == 8 && (nvec & 7) == 0;  // the 128 x 128 case: a thread's 64 pixels are one 8-byte LDS read
                                                       // (only when no thread's range is partial: a ragged tail takes the byte loop)
    if (one_word) {
        word = b0 + 8 <= nvec ? *reinterpret_cast<const unsigned long long *>(s_m8 + b0) : 0ull;
        cnt = __popcll(word);
    } else {
        for (int q = b0; q < b0 + bpt && q < nvec; q++) cnt += __popc((unsigned)s_m8[q]);
    }
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
    const int kept = total < maxp ? total : maxp;
    if (one_word) {
        while (word && rank < maxp) {
            const int bit = __ffsll((long long)word) - 1;
            word &= word - 1;
            s_pk[rank++] = (b0 << 3) + bit;
        }
    } else {
        for (int q = b0; q < b0 + bpt && q < nvec && rank < maxp; q++) {
            unsigned m = s_m8[q];
            while (m && rank < maxp) {
                const int j = __ffs(m) - 1;
                m &= m - 1;
                s_pk[rank++] = (q << 3) + j;
            }
        }
    }
    __syncthreads();
    stamp(stamps, wg, 2);

    // ---- A4: per-peak refinement, one wave per peak
    float4 *out = peaks + ((size_t)img * PP_NUM_PART + part) * maxp;
    for (int p = wave; p < kept; p += kWaves) {
        const int i = s_pk[p];
        const int py = i / w, px = i - py * w;
        float ox, oy, score;
        if (refine == 2) {
            // util.refine_centroid (utils/util.py:188-213), radius 2: border peaks are returned unrefined with the raw
            // score; otherwise offset = sum(box * grid) / sum(box) and score = mean(box).  np.mgrid makes x_grid vary
            // along ROWS, so the reference's "offset_x" is the row centroid; restated as written.  Sums in f64.
            if (py - 2 < 0 || py + 3 > h || px - 2 < 0 || px + 3 > w) {
                ox = (float)px;
                oy = (float)py;
                score = ldsf(smap, i);
            } else {
                double sx = 0.0, sy = 0.0, sv = 0.0;
                if (lane < 25) {
                    const int r = lane / 5, c = lane - r * 5;
                    const double v = (double)ldsf(smap, (py - 2 + r) * w + (px - 2 + c));
                    sx = v * (double)(r - 2);
                    sy = v * (double)(c - 2);
                    sv = v;
                }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    sx += __shfl_xor(sx, d);
                    sy += __shfl_xor(sy, d);
                    sv += __shfl_xor(sv, d);
                }
                ox = (float)((double)px + sx / sv);
                oy = (float)((double)py + sy / sv);
                score = (float)(sv / 25.0);
            }
        } else if (refine == 3) {
            ox = (float)px;
            oy = (float)py;
            score = ldsf(smap, i);
        } else if (refine == 1) {
            const int x_min = px - 2 < 0 ? 0 : px - 2, y_min = py - 2 < 0 ? 0 : py - 2;  // win_size 2, :135,:143-144
            const int x_max = px + 2 > w - 1 ? w - 1 : px + 2, y_max = py + 2 > h - 1 ? h - 1 : py + 2;
            const int pw = x_max - x_min + 1, ph = y_max - y_min + 1;
            const int uw = pw * 4, n = uw * ph * 4;
            // separable evaluation, same arithmetic as the per-pixel form: the horizontal pass of every patch row
            // is computed once (ph x uw values, kept in this wave's LDS scratch), the vertical pass reads 4 of them
            float *hp = s_hpass[wave];
            for (int k = lane; k < ph * uw; k += 64) {
                const int j = k / uw, col = k - j * uw;
                const int sx = ((col + 2) >> 2) - 1;
                const float4 ca = reinterpret_cast<const float4 *>(s_cub)[col & 3];
                const T *row = smap + (y_min + j) * w + x_min;
                float v = __fmul_rn(ldsf(row, clampi(sx - 1, 0, pw - 1)), ca.x);
                v = __fadd_rn(v, __fmul_rn(ldsf(row, clampi(sx, 0, pw - 1)), ca.y));
                v = __fadd_rn(v, __fmul_rn(ldsf(row, clampi(sx + 1, 0, pw - 1)), ca.z));
                v = __fadd_rn(v, __fmul_rn(ldsf(row, clampi(sx + 2, 0, pw - 1)), ca.w));
                hp[k] = v;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // this wave's LDS writes precede its reads below
            __builtin_amdgcn_wave_barrier();
            float best_v = -INFINITY;
            int best_k = 0x7fffffff;
            for (int k = lane; k < n; k += 64) {
                const int row = k / uw, col = k - row * uw;
                const int sy = ((row + 2) >> 2) - 1;
                const float4 cb = reinterpret_cast<const float4 *>(s_cub)[row & 3];
                float v = __fmul_rn(hp[clampi(sy - 1, 0, ph - 1) * uw + col], cb.x);
                v = __fadd_rn(v, __fmul_rn(hp[clampi(sy, 0, ph - 1) * uw + col], cb.y));
                v = __fadd_rn(v, __fmul_rn(hp[clampi(sy + 1, 0, ph - 1) * uw + col], cb.z));
                v = __fadd_rn(v, __fmul_rn(hp[clampi(sy + 2, 0, ph - 1) * uw + col], cb.w));
                if (v > best_v || best_k == 0x7fffffff) {
                    best_v = v;
                    best_k = k;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // arg-max with first-occurrence tie-break (ndarray.argmax, :156)
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ov = __shfl_xor(best_v, d);
                const int ok = __shfl_xor(best_k, d);
                if (ok != 0x7fffffff && (best_k == 0x7fffffff || ov > best_v || (ov == best_v && ok < best_k))) {
                    best_v = ov;
                    best_k = ok;
                }
            }
            const int row = best_k / uw, col = best_k - row * uw;
            ox = (float)(4 * x_min + col);  // :164-171 collapses to stride*x_min + col (exact integer)
            oy = (float)(4 * y_min + row);
            score = best_v;
        } else {
            ox = __fadd_rn(__fmul_rn(__fadd_rn((float)px, 0.5f), 4.0f), -0.5f);  // compute_resized_coords, :122-123
            oy = __fadd_rn(__fmul_rn(__fadd_rn((float)py, 0.5f), 4.0f), -0.5f);
            score = ldsf(smap, i);
        }
        if (lane == 0) out[p] = make_float4(ox, oy, score, 0.0f);
    }
    if (threadIdx.x == 0) {
        // write-through (sc1) so that the sorting workgroup below reads this launch's count; correctness never depends on it
        __hip_atomic_store(counts + img * PP_NUM_PART + part, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        status[img * kFlagWords + part] = total > maxp ? PP_ST_PEAK_OVERFLOW : 0u;  // plain store, every launch
    }
    __syncthreads();
    stamp(stamps, wg, 3);
    if (!order) return;
    // ---- the LAST workgroup of the grid orders the images by estimated matching load (sum over limbs of nA * nB), heaviest
    // first, for K_B's dispatch.  A stale count can only make the order worse, never wrong: the ranks below always form a
    // permutation of 0..B-1 (ties broken by index) because they are computed from ONE consistent copy in LDS.
    __shared__ int s_sorter;
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(arrive_all, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (int)(gridDim.x * gridDim.y) - 1;
        if (last) __hip_atomic_store(arrive_all, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
        s_sorter = last;
    }
    __syncthreads();
    if (!s_sorter) return;
    const int B = gridDim.y;
#ifndef PP_MAPS_HBM
    int *s_w = reinterpret_cast<int *>(lds_raw);  // the map is no longer needed (the host checked that B ints fit)
#else
    int *s_w = reinterpret_cast<int *>(s_m8 + ((((size_t)npix + 7) / 8 + 15) & ~(size_t)15));  // B ints of its own after the mask bytes
#endif
    for (int i = threadIdx.x; i < B; i += kThreads) {
        int c[PP_NUM_PART];
#pragma unroll
        for (int p = 0; p < PP_NUM_PART; p++) {
            const int v = __hip_atomic_load(counts + i * PP_NUM_PART + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c[p] = v < maxp ? v : maxp;
        }
        int wsum = 0;
#pragma unroll
        for (int l = 0; l < PP_NUM_LIMB; l++) wsum += c[kLimbA[l]] * c[kLimbB[l]];
        s_w[i] = wsum;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += kThreads) {
        const int wi = s_w[i];
        int rank = 0;
        for (int j = 0; j < B; j++) {
            const int wj = s_w[j];
            rank += (wj > wi) || (wj == wi && j < i);
        }
        order[rank] = i;
    }
}
#endif  // PP_INC_KA

#ifdef PP_INC_KB
#ifdef PP_MAPS_HBM
// The only global reads of the map are GlobalBicubicSampler's sixteen taps per sample: at() clamps the sample position to the x4
// map and bicubic4_at clamps every tap's row to [0, h) and column to [0, w) of the plane (window = the whole map), so each read
// lies inside the plane's h*w elements.  LDS layout (dynamic): [cubic 16 f32][LimbLds]; the assembly tail re-uses the region.
#define PP_LIMB_SAMPLER GlobalBicubicSampler
#define PP_LIMB_SAMPLER_INIT {ws + ((size_t)img * kWsChannels + limb) * ws_stride, s_cub, h, w}
#else
#define PP_LIMB_SAMPLER LdsBicubicSampler
#define PP_LIMB_SAMPLER_INIT {smap, s_cub, h, w, ld}
#endif
template <typename T, int NT>
#ifndef PP_MAPS_HBM
__global__ __launch_bounds__(NT, NT == 256 ? 3 : 4) void k_limb_connect(const T *__restrict__ net, int n_samples, int h, int w,
                                                           int flip, int maxp, int cap, int min_img_size,
                                                           const int *__restrict__ min_img_size_dev,
                                                           const float4 *__restrict__ peaks,
                                                           const int *__restrict__ counts, float4 *conns, float4 *aux,
                                                           int *conn_counts, unsigned *status, const int *__restrict__ order,
                                                           int *arrive, unsigned *ready, pp_record *records) {
#else
__global__ __launch_bounds__(NT, NT == 256 ? 3 : 4) void k_limb_connect_hbm(const T *__restrict__ ws, size_t ws_stride, int h, int w,
                                                               int maxp, int cap, int min_img_size,
                                                               const int *__restrict__ min_img_size_dev,
                                                               const float4 *__restrict__ peaks,
                                                               const int *__restrict__ counts, float4 *conns, float4 *aux,
                                                               int *conn_counts, unsigned *status,
                                                               const int *__restrict__ order, int *arrive, unsigned *ready,
                                                               pp_record *records) {
#endif
    extern __shared__ __align__(16) unsigned char lds_raw[];
    __shared__ int s_poff[PP_NUM_PART];
    const int limb = blockIdx.x, img = order ? order[blockIdx.y] : blockIdx.y;
    // Fused form (arrive != NULL): grid (31, B).  Workgroups 0..29 of an image match one limb each and PUBLISH it; workgroup 30
    // is the image's ASSEMBLY: one wave that consumes limb 0, 1, ... as each is published (the assembly needs them in this
    // order anyway, pafprocess.cpp:133), so it runs under the matching instead of after it.  arrive[img] is the image's
    // launch counter (touched by this kernel only): every workgroup of the image reads it at its start, limb l publishes
    // ready[img][l] = (counter + 1) << 8 | connection count, the assembly stores counter + 1 when it is done -- no flag is
    // ever reset and a flag of an earlier launch can never be mistaken for this launch's.  The assembly workgroup has the
    // HIGHEST index of its image: a workgroup is dispatched after every workgroup with a lower index of its XCD's queue, and
    // limb workgroups never wait, so everything it waits for is running or done (its polling is bounded nevertheless).
    const unsigned want = arrive ? (((unsigned)arrive[img] + 1u) & 0xffffffu) : 0u;
    if (limb == PP_NUM_LIMB) {
        if (threadIdx.x >= 64) return;
        __builtin_amdgcn_s_setprio(3);   // a lone latency-bound instruction stream next to streaming waves
        assemble_image_wave<true>(img, threadIdx.x, maxp, peaks + (size_t)img * PP_NUM_PART * maxp, counts + img * PP_NUM_PART,
                                  conns + (size_t)img * PP_NUM_LIMB * maxp, aux + (size_t)img * PP_NUM_LIMB * maxp,
                                  conn_counts + img * PP_NUM_LIMB, status, records + img, lds_raw,
                                  d_stamps ? d_stamps + (size_t)gridDim.x * gridDim.y * 8 : nullptr,  // diagnostics: after the limbs'
                                  ready + (size_t)img * PP_NUM_LIMB, want);
        if (threadIdx.x == 0) store_sc1(arrive + img, (int)want);
        return;
    }
    const int pa = d_limb_pairs[limb][0], pb = d_limb_pairs[limb][1];
    int nA = counts[img * PP_NUM_PART + pa], nB = counts[img * PP_NUM_PART + pb];
    nA = nA < maxp ? nA : maxp;
    nB = nB < maxp ? nB : maxp;
    int *cc = conn_counts + img * PP_NUM_LIMB + limb;
    long long *stamps = d_stamps;
    int ncn_out = 0;
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    if (nA == 0 || nB == 0) {  // no candidate pairs: no connections (pafprocess.cpp:56-58, :111)
        if (threadIdx.x == 0) {
            store_sc1(cc, 0);
            store_sc1(status + img * kFlagWords + PP_NUM_PART + limb, 0u);
        }
    } else {
#ifndef PP_MAPS_HBM
        const int ld = limb_map_ld<T>(w);   // padded LDS rows (see load_channel)
        size_t off = 0;
        T *smap = reinterpret_cast<T *>(lds_raw);
        off += (sizeof(T) * (size_t)h * ld + 15) & ~(size_t)15;
#else
        size_t off = 0;   // no map in LDS: the region starts at the cubic table
#endif
        float *s_cub = reinterpret_cast<float *>(lds_raw + off);
        off += 64;
        LimbLds L = carve_limb_lds(lds_raw + off, maxp, cap);

        if (threadIdx.x < 16) s_cub[threadIdx.x] = d_cubic4[threadIdx.x >> 2][threadIdx.x & 3];
        if (threadIdx.x < 64) {  // flat peak id of each part's first peak (pafprocess.cpp:43-48)
            int c = threadIdx.x < PP_NUM_PART ? counts[img * PP_NUM_PART + threadIdx.x] : 0;
            c = c < maxp ? c : maxp;
            int inc = c;
#pragma unroll
            for (int d = 1; d < 32; d <<= 1) {
                const int t = __shfl_up(inc, d);
                if ((int)threadIdx.x >= d) inc += t;
            }
            if (threadIdx.x < PP_NUM_PART) s_poff[threadIdx.x] = inc - c;
        }
        const float4 *pka = peaks + ((size_t)img * PP_NUM_PART + pa) * maxp;
        const float4 *pkb = peaks + ((size_t)img * PP_NUM_PART + pb) * maxp;
        for (int i = threadIdx.x; i < nA; i += NT) {
            const float4 p = pka[i];
            L.ax[i] = (int)p.x;  // Peak.x/y are ints: truncation (pafprocess.cpp:35-36)
            L.ay[i] = (int)p.y;
            L.as[i] = p.z;
        }
        for (int i = threadIdx.x; i < nB; i += NT) {
            const float4 p = pkb[i];
            L.bx[i] = (int)p.x;
            L.by[i] = (int)p.y;
            L.bs[i] = p.z;
        }
#ifndef PP_MAPS_HBM
        const size_t plane = (size_t)h * w;
        const T *o0 = net + ((size_t)img * n_samples * PP_NUM_CH + limb) * plane;
        const T *o1 = net + (((size_t)img * n_samples + 1) * PP_NUM_CH + d_flip_paf_ord[limb]) * plane;
        stamp(stamps, wg, 0);
        load_channel<NT>(smap, o0, o1, h, w, flip != 0, ld);
#else
        stamp(stamps, wg, 0);
#endif
        __syncthreads();
        stamp(stamps, wg, 1);

        PP_LIMB_SAMPLER<T> smp PP_LIMB_SAMPLER_INIT;
        const int mis = min_img_size_dev ? min_img_size_dev[img] : min_img_size;
        const size_t row = ((size_t)img * PP_NUM_LIMB + limb) * maxp;
        ncn_out = connect_limb<PP_LIMB_SAMPLER<T>, NT>(smp, L, nA, nB, cap, maxp, mis, conns + row, cc, status + img * kFlagWords + PP_NUM_PART + limb, stamps, wg,
                     aux + row, s_poff[pa], s_poff[pb]);
    }
    if (!arrive) return;  // two-kernel form (timing / diagnostics): k_assemble_wave follows as its own launch

    // ---- publish this limb.  Everything the assembly reads from this workgroup was stored write-through (store_sc1), so there
    // is no release fence: EVERY storing wave drains its stores, the workgroup meets at a barrier, one lane stores the flag.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) store_sc1(ready + (size_t)img * PP_NUM_LIMB + limb, (want << 8) | (unsigned)ncn_out);
}
#undef PP_LIMB_SAMPLER
#undef PP_LIMB_SAMPLER_INIT
#endif  // PP_INC_KB
