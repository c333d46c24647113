// kfdb.hip -- gfx950 KeyFrameDatabase: the per-entry work of DetectLoopCandidates /
// DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:76-309) as a forward scan
// over every stored BowVector, and the storage the scan reads.
//
//   k_kfdb_share   one wave per (query, stored keyframe): the shared-word count (mnLoopWords /
//                  mnRelocWords) and the index in the query of the first shared word, which
//                  orders lKFsSharingWords; excluded ids are masked
//   k_kfdb_max     maxCommonWords and the number of sharing keyframes, one workgroup per query
//   k_kfdb_select  minCommonWords = maxCommonWords * 0.8f, compaction of words > minCommonWords
//   k_kfdb_score   one workgroup per scored keyframe: L1Scoring::score, the terms in parallel into
//                  LDS, the double sum by one lane in ascending word order (the reference's
//                  merge order)
//   k_kfdb_move    entry-pool growth and compaction
#include <algorithm>
#include <cstring>

#include "kfdb.hpp"
#include "orb_common.hpp"

namespace orbgpu {

namespace {

constexpr int KF_T = 256;              // 4 waves
constexpr int KF_SLOTS_PER_BLOCK = 4;   // one keyframe per wave; the workgroup stages the query once
constexpr int KF_SCORE_BLOCKS = 256;   // per query; a block strides over the scored keyframes

struct KfdbQueryDev {
    int32_t woff, nq, eoff, nex;   // offsets into the staged word / excluded-id pools
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// index of w in the ascending s_q[0..nq), or -1
__device__ __forceinline__ int find_word(const uint32_t* s_q, int nq, uint32_t w) {
    int lo = 0, hi = nq;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_q[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return (lo < nq && s_q[lo] == w) ? lo : -1;
}

// find_word for four words at once: the branch-free form of the same search with a trip count
// that depends on nq alone (top = the largest power of two <= nq, 0 for an empty query), so the
// four chains of LDS reads overlap
__device__ __forceinline__ void find_words4(const uint32_t* s_q, int nq, int top, const uint32_t (&w)[4],
                                            int (&idx)[4]) {
    int pos[4] = {0, 0, 0, 0};   // words below w[k] found so far
    for (int step = top; step > 0; step >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int p = pos[k] + step;
            if (p <= nq && s_q[p - 1] < w[k]) pos[k] = p;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = (pos[k] < nq && s_q[pos[k]] == w[k]) ? pos[k] : -1;
}

__device__ __forceinline__ void stage_query(uint32_t* s_q, const uint32_t* qw, int nq) {
    for (int i = threadIdx.x; i < nq; i += KF_T) s_q[i] = qw[i];
    __syncthreads();
}

__global__ void __launch_bounds__(KF_T)
k_kfdb_share(const KfdbSlot* __restrict__ slots, int nslots, const uint32_t* __restrict__ pool_word,
             const KfdbQueryDev* __restrict__ qd, const uint32_t* __restrict__ q_word,
             const int32_t* __restrict__ q_excl, int stride, int32_t* __restrict__ words,
             int32_t* __restrict__ first) {
    __shared__ uint32_t s_q[kKfdbMaxWords];
    const int q = blockIdx.y;
    const KfdbQueryDev Q = qd[q];
    stage_query(s_q, q_word + Q.woff, Q.nq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* ex = q_excl + Q.eoff;
    const int top = Q.nq > 0 ? 1 << (31 - __clz(Q.nq)) : 0;
    for (int k = 0; k < KF_SLOTS_PER_BLOCK / 4; k++) {
        const int slot = blockIdx.x * KF_SLOTS_PER_BLOCK + k * 4 + wave;   // wave-uniform
        if (slot >= nslots) break;
        const KfdbSlot S = slots[slot];
        int cnt = 0, fst = 0x7fffffff;
        if (S.live) {
            int excluded = 0;
            for (int i = lane; i < Q.nex; i += 64) excluded |= ex[i] == S.id;
            if (!__any(excluded)) {
                const uint32_t* w = pool_word + S.off;
                for (int base = 0; base < S.len; base += 256) {   // four loads per lane in flight
                    uint32_t wk[4];
                    int idx[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int e = base + k * 64 + lane;
                        wk[k] = e < S.len ? w[e] : 0u;
                    }
                    find_words4(s_q, Q.nq, top, wk, idx);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        if (base + k * 64 + lane < S.len && idx[k] >= 0) {
                            cnt++;
                            fst = min(fst, idx[k]);
                        }
                }
                cnt = wave_sum(cnt);
                fst = wave_min(fst);
            }
        }
        if (lane == 0) {
            words[(size_t)q * stride + slot] = cnt;
            first[(size_t)q * stride + slot] = fst;
        }
    }
}

// maxCommonWords and the size of lKFsSharingWords of one query: one workgroup (integers: any order)
__global__ void __launch_bounds__(KF_T)
k_kfdb_max(int nslots, int stride, const int32_t* __restrict__ words, KfdbCounts* __restrict__ counts) {
    __shared__ int s_max[KF_T / 64], s_cnt[KF_T / 64];
    const int q = blockIdx.x;
    int m = 0, c = 0;
    for (int slot = threadIdx.x; slot < nslots; slot += KF_T) {
        const int w = words[(size_t)q * stride + slot];
        m = max(m, w);
        c += w > 0;
    }
    m = -wave_min(-m);
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) {
        s_max[threadIdx.x >> 6] = m;
        s_cnt[threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < KF_T / 64; i++) {
            m = max(m, s_max[i]);
            c += s_cnt[i];
        }
        counts[q].max_words = m;
        counts[q].n_sharing = c;
    }
}

__global__ void __launch_bounds__(KF_T)
k_kfdb_select(int nslots, int stride, const int32_t* __restrict__ words, KfdbCounts* __restrict__ counts,
              int32_t* __restrict__ scored_slot) {
    const int q = blockIdx.y, slot = blockIdx.x * KF_T + threadIdx.x;
    if (slot >= nslots) return;
    const int maxCommonWords = counts[q].max_words;
    const int minCommonWords = (int)((float)maxCommonWords * 0.8f);   // KeyFrameDatabase.cc:124, 240
    const int w = words[(size_t)q * stride + slot];
    if (w > 0 && w > minCommonWords) scored_slot[(size_t)q * stride + atomicAdd(&counts[q].n_scored, 1)] = slot;
}

__global__ void __launch_bounds__(KF_T)
k_kfdb_score(const KfdbSlot* __restrict__ slots, const uint32_t* __restrict__ pool_word,
             const double* __restrict__ pool_value, const KfdbQueryDev* __restrict__ qd,
             const uint32_t* __restrict__ q_word, const double* __restrict__ q_value, int stride,
             const int32_t* __restrict__ words, const int32_t* __restrict__ first,
             const KfdbCounts* __restrict__ counts, const int32_t* __restrict__ scored_slot,
             KfdbScored* __restrict__ out) {
    __shared__ uint32_t s_q[kKfdbMaxWords];
    __shared__ double s_term[kKfdbMaxWords];
    const int q = blockIdx.y;
    const int n_scored = counts[q].n_scored;
    if ((int)blockIdx.x >= n_scored) return;   // block-uniform
    const KfdbQueryDev Q = qd[q];
    stage_query(s_q, q_word + Q.woff, Q.nq);
    const double* qv = q_value + Q.woff;
    for (int r = blockIdx.x; r < n_scored; r += gridDim.x) {   // block-uniform
        const int slot = scored_slot[(size_t)q * stride + r];
        const KfdbSlot S = slots[slot];   // len <= kKfdbMaxWords
        const uint32_t* w = pool_word + S.off;
        const double* v = pool_value + S.off;
        // the terms of the shared words, all loads in flight together; a word the query lacks
        // contributes +0.0, which leaves the sum's bits as they are (no term and no partial sum
        // is -0.0: each is a difference of non-negative numbers rounded to nearest)
        for (int e = threadIdx.x; e < S.len; e += KF_T) {
            const int idx = find_word(s_q, Q.nq, w[e]);
            double term = 0;
            if (idx >= 0) {
                const double vi = qv[idx], wi = v[e];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);   // ScoringObject.cpp:21-66
            }
            s_term[e] = term;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // the stored words ascend with e: the reference's merge order
            double score = 0;
            for (int e = 0; e < S.len; e++) score += s_term[e];
            KfdbScored o;
            o.slot = slot;
            o.words = words[(size_t)q * stride + slot];
            o.first = first[(size_t)q * stride + slot];
            o.score = (float)(-score / 2.0);
            out[(size_t)q * stride + r] = o;
        }
        __syncthreads();
    }
}

// live keyframe i moves [src_off[i], +len[i]) of the old pool to [dst_off[i], ...) of the new one
__global__ void __launch_bounds__(KF_T)
k_kfdb_move(int n, const int32_t* __restrict__ src_off, const int32_t* __restrict__ dst_off,
            const int32_t* __restrict__ len, const uint32_t* __restrict__ src_word,
            const double* __restrict__ src_value, uint32_t* __restrict__ dst_word,
            double* __restrict__ dst_value) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int so = src_off[i], d = dst_off[i], m = len[i];
    for (int e = threadIdx.x; e < m; e += KF_T) {
        dst_word[d + e] = src_word[so + e];
        dst_value[d + e] = src_value[so + e];
    }
}

size_t al(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

KfDatabase::~KfDatabase() {
    if (s_) (void)hipStreamSynchronize(s_);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    if (d_slots_) (void)hipFree(d_slots_);
    if (d_word_) (void)hipFree(d_word_);
    if (d_value_) (void)hipFree(d_value_);
    if (d_stage_) (void)hipFree(d_stage_);
    if (d_work_) (void)hipFree(d_work_);
    if (d_counts_) (void)hipFree(d_counts_);
    if (h_stage_) (void)hipHostFree(h_stage_);
    if (h_counts_) (void)hipHostFree(h_counts_);
    if (h_scored_) (void)hipHostFree(h_scored_);
    if (s_) (void)hipStreamDestroy(s_);
}

int KfDatabase::init(int slots, int entries) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -4;
    ORB_HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    for (auto& e : ev_) ORB_HIP_CHECK(hipEventCreate(&e));
    slot_cap_ = std::max(slots, 1);
    pool_cap_ = std::max(entries, 1);
    ORB_HIP_CHECK(hipMalloc(&d_slots_, sizeof(KfdbSlot) * (size_t)slot_cap_));
    ORB_HIP_CHECK(hipMalloc(&d_word_, 4 * (size_t)pool_cap_));
    ORB_HIP_CHECK(hipMalloc(&d_value_, 8 * (size_t)pool_cap_));
    return 0;
}

// Move the live entries into a fresh pool of new_cap entries, holes squeezed out.
int KfDatabase::repack(long long new_cap) {
    if (new_cap > 0x7fffffffLL) return -3;
    std::vector<int32_t> tab;   // src_off | dst_off | len
    const int nl = (int)slot_of_.size();
    tab.resize(3 * (size_t)std::max(nl, 1));
    int i = 0;
    long long used = 0;
    for (size_t sl = 0; sl < slots_.size(); sl++) {
        KfdbSlot& S = slots_[sl];
        if (!S.live) continue;
        tab[i] = S.off;
        tab[nl + i] = (int32_t)used;
        tab[2 * nl + i] = S.len;
        S.off = (int32_t)used;
        used += S.len;
        i++;
    }
    uint32_t* nw = nullptr;
    double* nv = nullptr;
    int32_t* d_tab = nullptr;
    ORB_HIP_CHECK(hipMalloc(&nw, 4 * (size_t)new_cap));
    ORB_HIP_CHECK(hipMalloc(&nv, 8 * (size_t)new_cap));
    if (nl > 0) {
        ORB_HIP_CHECK(hipMalloc(&d_tab, 4 * tab.size()));
        ORB_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), 4 * tab.size(), hipMemcpyHostToDevice, s_));
        hipLaunchKernelGGL(k_kfdb_move, dim3(nl), dim3(KF_T), 0, s_, nl, d_tab, d_tab + nl, d_tab + 2 * nl, d_word_,
                           d_value_, nw, nv);
        ORB_HIP_CHECK(hipGetLastError());
    }
    ORB_HIP_CHECK(hipStreamSynchronize(s_));
    if (d_tab) (void)hipFree(d_tab);
    (void)hipFree(d_word_);
    (void)hipFree(d_value_);
    d_word_ = nw;
    d_value_ = nv;
    pool_cap_ = new_cap;
    pool_used_ = used;
    slots_dirty_ = true;
    return 0;
}

int KfDatabase::add(int count, const int32_t* id, const int32_t* start, const uint32_t* word, const double* value) {
    if (count <= 0) return 0;
    const long long tot = start[count] - start[0];
    if (live_entries_ + tot > 0x7fffffffLL) return -3;
    if (pool_used_ + tot > pool_cap_) {
        long long cap = pool_cap_;
        while (live_entries_ + tot > cap) cap *= 2;   // holes are squeezed out by the move
        if (cap > 0x7fffffffLL) cap = 0x7fffffffLL;
        if (int e = repack(cap)) return e;
    }
    // free slots first, then new ones; the table doubles when full
    const int fresh = std::max(0, count - (int)free_.size());
    if ((long long)slots_.size() + fresh > slot_cap_) {
        int cap = slot_cap_;
        while ((long long)slots_.size() + fresh > cap) cap *= 2;
        KfdbSlot* ns = nullptr;
        ORB_HIP_CHECK(hipMalloc(&ns, sizeof(KfdbSlot) * (size_t)cap));
        ORB_HIP_CHECK(hipStreamSynchronize(s_));
        (void)hipFree(d_slots_);
        d_slots_ = ns;
        slot_cap_ = cap;
    }
    if (tot > 0) {
        ORB_HIP_CHECK(hipMemcpyAsync(d_word_ + pool_used_, word + start[0], 4 * (size_t)tot, hipMemcpyHostToDevice, s_));
        ORB_HIP_CHECK(
            hipMemcpyAsync(d_value_ + pool_used_, value + start[0], 8 * (size_t)tot, hipMemcpyHostToDevice, s_));
        ORB_HIP_CHECK(hipStreamSynchronize(s_));   // the caller's arrays are free on return
    }
    for (int i = 0; i < count; i++) {
        int sl;
        if (!free_.empty()) {
            sl = free_.back();
            free_.pop_back();
        } else {
            sl = (int)slots_.size();
            slots_.push_back(KfdbSlot{});
            seq_.push_back(0);
        }
        const int len = start[i + 1] - start[i];
        slots_[sl] = KfdbSlot{id[i], (int32_t)(pool_used_ + (start[i] - start[0])), len, 1};
        seq_[sl] = next_seq_++;
        slot_of_[id[i]] = sl;
    }
    pool_used_ += tot;
    live_entries_ += tot;
    slots_dirty_ = true;
    return 0;
}

int KfDatabase::erase(int32_t id) {
    auto it = slot_of_.find(id);
    if (it == slot_of_.end()) return 0;
    const int sl = it->second;
    slots_[sl].live = 0;
    live_entries_ -= slots_[sl].len;
    free_.push_back(sl);
    slot_of_.erase(it);
    slots_dirty_ = true;
    // compact when the holes exceed the live entries
    if (pool_used_ - live_entries_ > live_entries_) return repack(pool_cap_);
    return 0;
}

int KfDatabase::clear() {
    slots_.clear();
    seq_.clear();
    free_.clear();
    slot_of_.clear();
    pool_used_ = live_entries_ = 0;
    slots_dirty_ = true;
    return 0;
}

int KfDatabase::reserve_query(int count, size_t stage_bytes) {
    if (stage_bytes > stage_cap_) {
        ORB_HIP_CHECK(hipStreamSynchronize(s_));
        if (h_stage_) (void)hipHostFree(h_stage_);
        if (d_stage_) (void)hipFree(d_stage_);
        h_stage_ = d_stage_ = nullptr;
        stage_cap_ = 0;
        const size_t cap = std::max(stage_bytes * 2, (size_t)1 << 16);
        ORB_HIP_CHECK(hipHostMalloc((void**)&h_stage_, cap, hipHostMallocDefault));
        ORB_HIP_CHECK(hipMalloc(&d_stage_, cap));
        stage_cap_ = cap;
    }
    if (count > q_cap_ || slot_cap_ > q_stride_) {
        ORB_HIP_CHECK(hipStreamSynchronize(s_));
        if (d_work_) (void)hipFree(d_work_);
        if (d_counts_) (void)hipFree(d_counts_);
        if (h_counts_) (void)hipHostFree(h_counts_);
        if (h_scored_) (void)hipHostFree(h_scored_);
        d_work_ = nullptr;
        d_counts_ = h_counts_ = nullptr;
        h_scored_ = nullptr;
        q_cap_ = q_stride_ = 0;
        const int qc = std::max(count, 1), st = slot_cap_;
        const size_t cells = (size_t)qc * st;
        ORB_HIP_CHECK(hipMalloc(&d_work_, 3 * 4 * cells));
        ORB_HIP_CHECK(hipMalloc(&d_counts_, sizeof(KfdbCounts) * (size_t)qc));
        ORB_HIP_CHECK(hipHostMalloc((void**)&h_counts_, sizeof(KfdbCounts) * (size_t)qc, hipHostMallocDefault));
        ORB_HIP_CHECK(hipHostMalloc((void**)&h_scored_, sizeof(KfdbScored) * cells, hipHostMallocDefault));
        q_cap_ = qc;
        q_stride_ = st;
    }
    return 0;
}

int KfDatabase::query(int count, const KfdbQuery* q) {
    timed_ = false;
    if (count <= 0) return 0;
    const int nslots = (int)slots_.size();
    // staging block: descriptors | words | excluded ids | values
    size_t nw = 0, ne = 0;
    for (int i = 0; i < count; i++) {
        nw += (size_t)q[i].nq;
        ne += (size_t)q[i].n_exclude;
    }
    const size_t o_word = al(sizeof(KfdbQueryDev) * (size_t)count), o_excl = o_word + al(4 * nw),
                 o_val = o_excl + al(4 * ne), bytes = o_val + al(8 * nw);
    if (int e = reserve_query(count, bytes)) return e;
    if (nslots == 0) {   // an empty database shares nothing
        std::memset(h_counts_, 0, sizeof(KfdbCounts) * (size_t)count);
        return 0;
    }
    KfdbQueryDev* qd = (KfdbQueryDev*)h_stage_;
    uint32_t* hw = (uint32_t*)(h_stage_ + o_word);
    int32_t* he = (int32_t*)(h_stage_ + o_excl);
    double* hv = (double*)(h_stage_ + o_val);
    size_t w = 0, x = 0;
    for (int i = 0; i < count; i++) {
        qd[i] = KfdbQueryDev{(int32_t)w, q[i].nq, (int32_t)x, q[i].n_exclude};
        if (q[i].nq > 0) {
            std::memcpy(hw + w, q[i].word, 4 * (size_t)q[i].nq);
            std::memcpy(hv + w, q[i].value, 8 * (size_t)q[i].nq);
        }
        if (q[i].n_exclude > 0) std::memcpy(he + x, q[i].exclude, 4 * (size_t)q[i].n_exclude);
        w += (size_t)q[i].nq;
        x += (size_t)q[i].n_exclude;
    }
    if (slots_dirty_) {
        ORB_HIP_CHECK(
            hipMemcpyAsync(d_slots_, slots_.data(), sizeof(KfdbSlot) * (size_t)nslots, hipMemcpyHostToDevice, s_));
        ORB_HIP_CHECK(hipStreamSynchronize(s_));   // slots_ is pageable and changes with the next add
        slots_dirty_ = false;
    }
    ORB_HIP_CHECK(hipMemcpyAsync(d_stage_, h_stage_, bytes, hipMemcpyHostToDevice, s_));
    ORB_HIP_CHECK(hipMemsetAsync(d_counts_, 0, sizeof(KfdbCounts) * (size_t)count, s_));
    const KfdbQueryDev* d_qd = (const KfdbQueryDev*)d_stage_;
    const uint32_t* d_qw = (const uint32_t*)(d_stage_ + o_word);
    const int32_t* d_qe = (const int32_t*)(d_stage_ + o_excl);
    const double* d_qv = (const double*)(d_stage_ + o_val);
    const size_t cells = (size_t)q_cap_ * q_stride_;
    int32_t* d_words = d_work_;
    int32_t* d_first = d_work_ + cells;
    int32_t* d_sslot = d_work_ + 2 * cells;
    const unsigned gs = (unsigned)((nslots + KF_SLOTS_PER_BLOCK - 1) / KF_SLOTS_PER_BLOCK);
    if (timing_) ORB_HIP_CHECK(hipEventRecord(ev_[0], s_));
    hipLaunchKernelGGL(k_kfdb_share, dim3(gs, count), dim3(KF_T), 0, s_, d_slots_, nslots, d_word_, d_qd, d_qw, d_qe,
                       q_stride_, d_words, d_first);
    hipLaunchKernelGGL(k_kfdb_max, dim3(count), dim3(KF_T), 0, s_, nslots, q_stride_, d_words, d_counts_);
    hipLaunchKernelGGL(k_kfdb_select, dim3((nslots + KF_T - 1) / KF_T, count), dim3(KF_T), 0, s_, nslots, q_stride_,
                       d_words, d_counts_, d_sslot);
    if (timing_) ORB_HIP_CHECK(hipEventRecord(ev_[1], s_));
    hipLaunchKernelGGL(k_kfdb_score, dim3(std::min(nslots, KF_SCORE_BLOCKS), count), dim3(KF_T), 0, s_, d_slots_, d_word_, d_value_, d_qd, d_qw, d_qv,
                       q_stride_, d_words, d_first, d_counts_, d_sslot, h_scored_);
    ORB_HIP_CHECK(hipGetLastError());
    if (timing_) ORB_HIP_CHECK(hipEventRecord(ev_[2], s_));
    ORB_HIP_CHECK(hipMemcpyAsync(h_counts_, d_counts_, sizeof(KfdbCounts) * (size_t)count, hipMemcpyDeviceToHost, s_));
    ORB_HIP_CHECK(hipStreamSynchronize(s_));
    if (timing_) {
        ORB_HIP_CHECK(hipEventElapsedTime(&ms_[0], ev_[0], ev_[1]));
        ORB_HIP_CHECK(hipEventElapsedTime(&ms_[1], ev_[1], ev_[2]));
        timed_ = true;
    }
    return 0;
}

}  // namespace orbgpu
