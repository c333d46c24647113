// map.hip -- gfx950 Map: the observation relation, the covisibility vote and
// Tracking::UpdateLocalMap (reference src/Tracking.cc:1195-1339, src/KeyFrame.cc UpdateConnections).
//
//   k_map_csr_count / k_map_csr_scan / k_map_csr_fill
//                    the inverse index map point -> keyframe slots over the observed cells; the
//                    fill takes its places with atomics: the order inside a point's list is
//                    never observable, only integer counts are formed from it
//   k_map_vote       one workgroup per query: every entry of the list walks its point's slot
//                    list and adds 1 to the slot's counter with integer atomics, in LDS up to
//                    kMapLdsSlots keyframe slots and in device memory above
//   k_map_select     UpdateLocalKeyFrames: the voted keyframes compacted in ascending id order
//                    (block prefix scan over the by-id permutation), the first strict maximum,
//                    then one lane replays the extension loop with its three breaks
//   k_map_pt_min / k_map_pt_count / k_map_pt_scan / k_map_pt_write
//                    UpdateLocalPoints: first occurrence = atomicMin of the concatenated position
//                    (list index * 4096 + slot) per point, ordered compaction per row
//   k_map_remap      cur_row, row and the gather of the global table's rows
//   k_map_restore    the touched scratch entries back to idle
#include <algorithm>
#include <cstring>
#include <utility>

#include "map.hpp"
#include "orb_common.hpp"

namespace orbgpu {

namespace {

constexpr int MT = 256;        // 4 waves
constexpr int MV = 512;        // the vote: one list entry per thread, up to 8 passes
constexpr int MSCAN = 1024;    // the index scan: one workgroup
constexpr int kIdle = 0x7fffffff;

__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive prefix of v over the workgroup (NT threads) and the total; s_w holds NT / 64 ints
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = wave_incl_scan(v);
    __syncthreads();   // s_w may still be read from the previous call
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) {
        const int t = s_w[w];
        if (w < wave) base += t;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

__global__ void __launch_bounds__(MT)
k_map_csr_count(const MapSlotDev* __restrict__ slots, const int32_t* __restrict__ order,
                const int32_t* __restrict__ mp, const uint8_t* __restrict__ obs, int npts,
                int32_t* __restrict__ pt_cnt) {
    const MapSlotDev S = slots[order[blockIdx.x]];
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        if (p >= 0 && p < npts && obs[S.off + i]) atomicAdd(&pt_cnt[p], 1);
    }
}

// pt_start[0 .. npts] = exclusive scan of pt_cnt[0 .. npts), in place; cursor = a copy
__global__ void __launch_bounds__(MSCAN)
k_map_csr_scan(int npts, int32_t* __restrict__ pt_start, int32_t* __restrict__ cursor) {
    __shared__ int s_w[MSCAN / 64];
    const int per = (npts + MSCAN - 1) / MSCAN;
    const int lo = min(npts, (int)threadIdx.x * per), hi = min(npts, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += pt_start[i];
    int total;
    int run = block_excl_scan<MSCAN>(sum, s_w, &total);
    for (int i = lo; i < hi; i++) {
        const int c = pt_start[i];
        pt_start[i] = run;
        cursor[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) pt_start[npts] = total;
}

__global__ void __launch_bounds__(MT)
k_map_csr_fill(const MapSlotDev* __restrict__ slots, const int32_t* __restrict__ order,
               const int32_t* __restrict__ mp, const uint8_t* __restrict__ obs, int npts,
               int32_t* __restrict__ cursor, int32_t* __restrict__ pt_list) {
    const int slot = order[blockIdx.x];
    const MapSlotDev S = slots[slot];
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        if (p >= 0 && p < npts && obs[S.off + i]) pt_list[atomicAdd(&cursor[p], 1)] = slot;
    }
}

// Q: the queries of the launch (a MapQueryDev every `qstride` bytes).  LDS: the counters of
// this query live in dynamic LDS and are stored once at the end; otherwise cnt's row was zeroed
// before the launch and takes the atomics itself.
template <bool LDS>
__global__ void __launch_bounds__(MV)
k_map_vote(const uint8_t* __restrict__ Q, size_t qstride, const int32_t* __restrict__ pt_start,
           const int32_t* __restrict__ pt_list, int npts, int nslots, int stride, int32_t* __restrict__ cnt) {
    extern __shared__ int s_cnt[];
    const MapQueryDev q = *(const MapQueryDev*)(Q + qstride * blockIdx.x);
    int32_t* out = cnt + (size_t)blockIdx.x * stride;
    int* c = LDS ? s_cnt : out;
    if (LDS) {
        for (int i = threadIdx.x; i < nslots; i += MV) s_cnt[i] = 0;
        __syncthreads();
    }
    for (int e = threadIdx.x; e < q.n; e += MV) {
        const int p = q.list[e];
        if (p < 0) continue;
        if (q.bad && p < q.nbad && q.bad[p]) {   // Tracking.cc:1254: mvpMapPoints[i] = NULL
            q.list[e] = -1;
            continue;
        }
        if (p >= npts) continue;   // never observed
        const int hi = pt_start[p + 1];
        for (int k = pt_start[p]; k < hi; k++) {
            const int slot = pt_list[k];
            if (slot != q.exclude) atomicAdd(&c[slot], 1);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nslots; i += MV) out[i] = s_cnt[i];
    }
}

__device__ __forceinline__ int live_slot(const int32_t* id2slot, int nid, int id) {
    return (id >= 0 && id < nid) ? id2slot[id] : -1;
}

// UpdateLocalKeyFrames after the vote (Tracking.cc:1262-1339) of frame blockIdx.x.
// cnt: > 0 voted; the extension marks what it appends with -1 (mnTrackReferenceForFrame).
__global__ void __launch_bounds__(MT)
k_map_select(const MapLocalDev* __restrict__ F, const int32_t* __restrict__ order, int n_live,
             const MapSlotDev* __restrict__ slots, const MapNbDev* __restrict__ nb,
             const int32_t* __restrict__ child, const int32_t* __restrict__ id2slot, int nid, int stride,
             int32_t* __restrict__ cnt_all, int32_t* __restrict__ kfslot_all) {
    __shared__ int s_w[MT / 64];
    __shared__ int s_best[MT], s_pos[MT];
    const MapLocalDev f = F[blockIdx.x];
    int32_t* cnt = cnt_all + (size_t)blockIdx.x * stride;
    int32_t* kfslot = kfslot_all + (size_t)blockIdx.x * stride;
    int base = 0, best = 0, bpos = kIdle;
    for (int t0 = 0; t0 < n_live; t0 += MT) {   // block-uniform
        const int t = t0 + threadIdx.x;
        int slot = -1, c = 0;
        if (t < n_live) {
            slot = order[t];
            c = cnt[slot];
        }
        int total;
        const int r = base + block_excl_scan<MT>(c > 0, s_w, &total);
        if (c > 0) {
            kfslot[r] = slot;
            if (r < f.kf_cap) f.local_kf[r] = slots[slot].id;
            if (c > best) {   // positions ascend within a thread: the first strict maximum
                best = c;
                bpos = r;
            }
        }
        base += total;
    }
    s_best[threadIdx.x] = best;
    s_pos[threadIdx.x] = bpos;
    __syncthreads();   // also orders the kfslot stores before lane 0's loads
    if (threadIdx.x != 0) return;
    for (int i = 1; i < MT; i++)
        if (s_best[i] > best || (s_best[i] == best && s_pos[i] < bpos)) {
            best = s_best[i];
            bpos = s_pos[i];
        }
    MapCounts out = {0, -1, 0, 0};
    const int voted = base;
    if (voted > 0) {
        out.ref_kf = slots[kfslot[bpos]].id;
        int n = voted;
        for (int t = 0; t < voted; t++) {   // the end iterator is fixed before the loop
            if (n > kMapKfStop) break;
            const MapNbDev N = nb[kfslot[t]];
            for (int k = 0; k < N.ncov; k++) {
                const int s2 = live_slot(id2slot, nid, N.cov[k]);
                if (s2 >= 0 && cnt[s2] == 0) {
                    cnt[s2] = -1;
                    kfslot[n] = s2;
                    if (n < f.kf_cap) f.local_kf[n] = N.cov[k];
                    n++;
                    break;
                }
            }
            for (int k = 0; k < N.nchild; k++) {
                const int cid = child[N.child_off + k];
                const int s2 = live_slot(id2slot, nid, cid);
                if (s2 >= 0 && cnt[s2] == 0) {
                    cnt[s2] = -1;
                    kfslot[n] = s2;
                    if (n < f.kf_cap) f.local_kf[n] = cid;
                    n++;
                    break;
                }
            }
            const int sp = live_slot(id2slot, nid, N.parent);
            if (sp >= 0 && cnt[sp] == 0) {
                cnt[sp] = -1;
                kfslot[n] = sp;
                if (n < f.kf_cap) f.local_kf[n] = N.parent;
                n++;
                break;   // Tracking.cc:1329: this break leaves the loop over the keyframes
            }
        }
        out.n_kf = n;
    }
    *f.counts = out;
}

__device__ __forceinline__ bool pt_ok(const MapQueryDev& q, int p, int nscr) {
    return p >= 0 && p < nscr && !(q.bad && p < q.nbad && q.bad[p]);
}

// grid (keyframe of the list, frame)
__global__ void __launch_bounds__(MT)
k_map_pt_min(const MapLocalDev* __restrict__ F, const MapSlotDev* __restrict__ slots,
             const int32_t* __restrict__ mp, int stride, const int32_t* __restrict__ kfslot_all,
             int nscr, int32_t* __restrict__ scr_all) {
    const MapLocalDev f = F[blockIdx.y];
    const int k = blockIdx.x;
    if (k >= f.counts->n_kf) return;
    const MapSlotDev S = slots[kfslot_all[(size_t)blockIdx.y * stride + k]];
    int32_t* scr = scr_all + (size_t)blockIdx.y * nscr;
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        if (pt_ok(f.q, p, nscr)) atomicMin(&scr[p], k * kMapMaxRow + i);
    }
}

__global__ void __launch_bounds__(MT)
k_map_pt_count(const MapLocalDev* __restrict__ F, const MapSlotDev* __restrict__ slots,
               const int32_t* __restrict__ mp, int stride, const int32_t* __restrict__ kfslot_all,
               int nscr, const int32_t* __restrict__ scr_all, int32_t* __restrict__ rowcnt_all) {
    __shared__ int s_w[MT / 64];
    const MapLocalDev f = F[blockIdx.y];
    const int k = blockIdx.x;
    if (k >= f.counts->n_kf) return;
    const MapSlotDev S = slots[kfslot_all[(size_t)blockIdx.y * stride + k]];
    const int32_t* scr = scr_all + (size_t)blockIdx.y * nscr;
    int c = 0;
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        c += pt_ok(f.q, p, nscr) && scr[p] == k * kMapMaxRow + i;
    }
    int total;
    (void)block_excl_scan<MT>(c, s_w, &total);
    if (threadIdx.x == 0) rowcnt_all[(size_t)blockIdx.y * stride + k] = total;
}

// one workgroup per frame: rowoff = exclusive scan of rowcnt over the list, n_pt = the total
__global__ void __launch_bounds__(MT)
k_map_pt_scan(const MapLocalDev* __restrict__ F, int stride, const int32_t* __restrict__ rowcnt_all,
              int32_t* __restrict__ rowoff_all) {
    __shared__ int s_w[MT / 64];
    const MapLocalDev f = F[blockIdx.x];
    const int n_kf = f.counts->n_kf;
    const int32_t* rowcnt = rowcnt_all + (size_t)blockIdx.x * stride;
    int32_t* rowoff = rowoff_all + (size_t)blockIdx.x * stride;
    int base = 0;
    for (int t0 = 0; t0 < n_kf; t0 += MT) {
        const int t = t0 + threadIdx.x;
        const int c = t < n_kf ? rowcnt[t] : 0;
        int total;
        const int r = base + block_excl_scan<MT>(c, s_w, &total);
        if (t < n_kf) rowoff[t] = r;
        base += total;
    }
    if (threadIdx.x == 0) f.counts->n_pt = base;
}

// the kept cells of one row in slot order; a kept point's scratch entry becomes -(local row + 1)
__global__ void __launch_bounds__(MT)
k_map_pt_write(const MapLocalDev* __restrict__ F, const MapSlotDev* __restrict__ slots,
               const int32_t* __restrict__ mp, int stride, const int32_t* __restrict__ kfslot_all,
               const int32_t* __restrict__ rowoff_all, int nscr, int32_t* __restrict__ scr_all) {
    __shared__ int s_w[MT / 64];
    const MapLocalDev f = F[blockIdx.y];
    const int k = blockIdx.x;
    if (k >= f.counts->n_kf) return;
    const MapSlotDev S = slots[kfslot_all[(size_t)blockIdx.y * stride + k]];
    int32_t* scr = scr_all + (size_t)blockIdx.y * nscr;
    int base = rowoff_all[(size_t)blockIdx.y * stride + k];
    for (int i0 = 0; i0 < S.n; i0 += MT) {   // block-uniform
        const int i = i0 + threadIdx.x;
        int p = -1;
        bool keep = false;
        if (i < S.n) {
            p = mp[S.off + i];
            keep = pt_ok(f.q, p, nscr) && scr[p] == k * kMapMaxRow + i;
        }
        int total;
        const int j = base + block_excl_scan<MT>(keep, s_w, &total);
        if (keep) {
            if (j < f.pt_cap) f.local_mp[j] = p;
            scr[p] = -(j + 1);
        }
        base += total;
    }
}

// grid (ceil(max(N, pt_cap) / MT), frame)
__global__ void __launch_bounds__(MT)
k_map_remap(const MapLocalDev* __restrict__ F, int nscr, const int32_t* __restrict__ scr_all) {
    const MapLocalDev f = F[blockIdx.y];
    if (f.counts->n_kf == 0) return;   // the reference returns early: the outputs stay
    const int32_t* scr = scr_all + (size_t)blockIdx.y * nscr;
    const int t = blockIdx.x * MT + threadIdx.x;
    if (t < f.q.n) {
        const int p = f.q.list[t];
        int r = -1;
        if (p >= 0 && p < nscr) {
            const int v = scr[p];
            if (v < 0 && -(v + 1) < f.pt_cap) r = -(v + 1);
        }
        f.cur_row[t] = r;
    }
    if (t >= f.pt_cap) return;
    const int n_pt = f.counts->n_pt;
    if (t >= n_pt) {
        if (f.pad_rows) {
            if (f.row) f.row[t] = -1;
            if (f.g_skip) f.g_skip[t] = 1;
        }
        return;
    }
    const int p = f.local_mp[t];
    if (f.row) f.row[t] = p;
    if (!f.g_skip) return;
    if (p >= f.t_n) {   // the table has no such row
        f.g_skip[t] = 1;
        return;
    }
    f.g_skip[t] = 0;
    for (int c = 0; c < 3; c++) {
        f.g_pos[3 * (size_t)t + c] = f.t_pos[3 * (size_t)p + c];
        f.g_normal[3 * (size_t)t + c] = f.t_normal[3 * (size_t)p + c];
    }
    const uint8_t* sd = f.t_desc + 32 * (size_t)p;
    uint8_t* dd = f.g_desc + 32 * (size_t)t;
    if ((((uintptr_t)sd | (uintptr_t)dd) & 15) == 0) {   // rows of aligned tables: two 16-byte moves
        const uint4 a = ((const uint4*)sd)[0], b = ((const uint4*)sd)[1];
        ((uint4*)dd)[0] = a;
        ((uint4*)dd)[1] = b;
    } else {
        for (int c = 0; c < 32; c++) dd[c] = sd[c];
    }
    f.g_obs[t] = f.t_obs[p];
    f.g_maxd[t] = f.t_maxd[p];
    f.g_mind[t] = f.t_mind[p];
}

__global__ void __launch_bounds__(MT)
k_map_restore(const MapLocalDev* __restrict__ F, const MapSlotDev* __restrict__ slots,
              const int32_t* __restrict__ mp, int stride, const int32_t* __restrict__ kfslot_all,
              int nscr, int32_t* __restrict__ scr_all) {
    const MapLocalDev f = F[blockIdx.y];
    const int k = blockIdx.x;
    if (k >= f.counts->n_kf) return;
    const MapSlotDev S = slots[kfslot_all[(size_t)blockIdx.y * stride + k]];
    int32_t* scr = scr_all + (size_t)blockIdx.y * nscr;
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        if (p >= 0 && p < nscr) scr[p] = kIdle;
    }
}

__global__ void __launch_bounds__(MT) k_map_fill(int32_t* __restrict__ a, size_t n, int32_t v) {
    for (size_t i = (size_t)blockIdx.x * MT + threadIdx.x; i < n; i += (size_t)gridDim.x * MT) a[i] = v;
}

// ---------------------------------------------------------------- culling
// LocalMapping::KeyFrameCulling (LocalMapping.cc) and MapPointCulling over the handle.
//   k_cull_index   the observing cells of every point (slot * 4096 + index) in the places of
//                  pt_start, and nObs; same predicate as k_map_csr_count, so the ranges agree
//   k_cull_count   one workgroup per candidate: nMPs / nRedundant against the initial state
//   k_cull_walk    one workgroup walks the candidates in order; from the first cull on it counts
//                  each later candidate again against dead[] and scr[], and on a cull takes the
//                  row's observations off nObs and compacts the points that went bad in slot order
//   k_cull_points  MapPointCulling, one point per thread

constexpr int kCullBad = 1 << 30;   // scr: the point went bad in this call

struct CullDev {
    const MapSlotDev* slots;
    const int32_t* mp;
    const uint8_t* obs;
    const uint8_t* oct;
    const uint8_t* flags;
    const int32_t* pt_start;
    const uint32_t* pt_obs;
    const int32_t* nobs;
    int32_t* scr;            // written and read again inside k_cull_walk
    uint8_t* dead;           // the same
    const uint8_t* bad;
    int32_t nbad, monocular;
};

__global__ void __launch_bounds__(MT)
k_cull_index(const MapSlotDev* __restrict__ slots, const int32_t* __restrict__ order,
             const int32_t* __restrict__ mp, const uint8_t* __restrict__ obs, const uint8_t* __restrict__ flags,
             int npts, int32_t* __restrict__ cursor, uint32_t* __restrict__ pt_obs, int32_t* __restrict__ nobs) {
    const int slot = order[blockIdx.x];
    const MapSlotDev S = slots[slot];
    for (int i = threadIdx.x; i < S.n; i += MT) {
        const int p = mp[S.off + i];
        if (p >= 0 && p < npts && obs[S.off + i]) {
            pt_obs[atomicAdd(&cursor[p], 1)] = (uint32_t)slot * kMapMaxRow + (uint32_t)i;
            atomicAdd(&nobs[p], (flags[S.off + i] & kMapKeyStereo) ? 2 : 1);
        }
    }
}

// slot i of the candidate's row S (keyframe slot `slot`): LocalMapping.cc KeyFrameCulling's loop body
__device__ __forceinline__ void cull_count_cell(const CullDev& C, int slot, const MapSlotDev& S, int i, int& nmps,
                                                int& nred) {
    const int cell = S.off + i;
    const int p = C.mp[cell];
    if (p < 0) return;
    if (C.bad && p < C.nbad && C.bad[p]) return;
    const int sc = C.scr[p];
    if (sc & kCullBad) return;
    if (!C.monocular && (C.flags[cell] & kMapKeyFar)) return;
    nmps++;
    if (C.nobs[p] - sc <= 3) return;   // pMP->Observations() > thObs
    const int level = C.oct[cell];
    const int hi = C.pt_start[p + 1];
    int n = 0;
    for (int k = C.pt_start[p]; k < hi && n < 3; k++) {
        const uint32_t code = C.pt_obs[k];
        const int s2 = (int)(code / kMapMaxRow);
        if (s2 == slot || C.dead[s2]) continue;
        if ((int)C.oct[C.slots[s2].off + (int)(code % kMapMaxRow)] <= level + 1) n++;
    }
    nred += n >= 3;
}

__global__ void __launch_bounds__(MT)
k_cull_count(CullDev C, const int32_t* __restrict__ cand_slot, int32_t* __restrict__ nmps, int32_t* __restrict__ nred) {
    __shared__ int s_w[MT / 64];
    const int slot = cand_slot[blockIdx.x];
    int a = 0, b = 0;
    if (slot >= 0) {
        const MapSlotDev S = C.slots[slot];
        for (int i = threadIdx.x; i < S.n; i += MT) cull_count_cell(C, slot, S, i, a, b);
    }
    int ta, tb;
    (void)block_excl_scan<MT>(a, s_w, &ta);
    (void)block_excl_scan<MT>(b, s_w, &tb);
    if (threadIdx.x == 0) {
        nmps[blockIdx.x] = ta;
        nred[blockIdx.x] = tb;
    }
}

// nmps / nred hold k_cull_count's answers on entry
__global__ void __launch_bounds__(MT)
k_cull_walk(CullDev C, int n, const int32_t* __restrict__ cand_slot, const uint8_t* __restrict__ not_erase,
            int cap_bad, int32_t* nmps, int32_t* nred, int32_t* __restrict__ verdict, int32_t* __restrict__ bad_mp,
            int32_t* __restrict__ n_bad) {
    __shared__ int s_w[MT / 64];
    int nout = 0;
    bool culled = false;
    for (int c = 0; c < n; c++) {   // everything that steers the loop is block-uniform
        const int slot = cand_slot[c];
        if (slot < 0) {
            if (threadIdx.x == 0) {
                verdict[c] = 3;
                nmps[c] = 0;
                nred[c] = 0;
            }
            continue;
        }
        const MapSlotDev S = C.slots[slot];
        int ta, tb;
        if (!culled) {
            ta = nmps[c];
            tb = nred[c];
        } else {
            int a = 0, b = 0;
            for (int i = threadIdx.x; i < S.n; i += MT) cull_count_cell(C, slot, S, i, a, b);
            (void)block_excl_scan<MT>(a, s_w, &ta);
            (void)block_excl_scan<MT>(b, s_w, &tb);
            if (threadIdx.x == 0) {
                nmps[c] = ta;
                nred[c] = tb;
            }
        }
        int v = 0;
        if ((double)tb > 0.9 * (double)ta) v = (not_erase && not_erase[c]) ? 2 : 1;
        if (threadIdx.x == 0) verdict[c] = v;
        if (v != 1) continue;
        // KeyFrame::SetBadFlag: EraseObservation(this) of every slot, in slot order
        culled = true;
        if (threadIdx.x == 0) C.dead[slot] = 1;
        for (int i0 = 0; i0 < S.n; i0 += MT) {
            const int i = i0 + (int)threadIdx.x;
            int p = -1;
            bool newly = false;
            if (i < S.n && C.obs[S.off + i]) {
                p = C.mp[S.off + i];
                if (p >= 0) {   // a row holds a point once: no two lanes share p
                    int sc = C.scr[p];
                    if (!(sc & kCullBad)) {
                        sc += (C.flags[S.off + i] & kMapKeyStereo) ? 2 : 1;
                        if (C.nobs[p] - sc <= 2) {   // MapPoint::EraseObservation: nObs <= 2 -> SetBadFlag
                            sc |= kCullBad;
                            newly = true;
                        }
                        C.scr[p] = sc;
                    }
                }
            }
            int total;
            const int r = nout + block_excl_scan<MT>(newly, s_w, &total);
            if (newly && r < cap_bad) bad_mp[r] = p;
            nout += total;
        }
        __syncthreads();   // scr and dead of this cull before the next candidate's count
    }
    if (threadIdx.x == 0) *n_bad = nout;
}

__global__ void __launch_bounds__(MT)
k_cull_points(int n, const int32_t* __restrict__ mp, const int32_t* __restrict__ first_kf,
              const int32_t* __restrict__ found, const int32_t* __restrict__ visible, const uint8_t* __restrict__ bad,
              int nbad, const int32_t* __restrict__ nobs, int npts, int cur_kf, int th_obs,
              int32_t* __restrict__ verdict, int32_t* __restrict__ observations) {
    const int t = blockIdx.x * MT + threadIdx.x;
    if (t >= n) return;
    const int p = mp[t];
    const int no = p < npts ? nobs[p] : 0;   // never observed
    const int age = cur_kf - first_kf[t];
    int v = 0;
    if (bad && p < nbad && bad[p]) v = 1;
    else if ((float)found[t] / (float)visible[t] < 0.25f) v = 2;   // MapPoint::GetFoundRatio
    else if (age >= 2 && no <= th_obs) v = 3;
    else if (age >= 3) v = 4;
    verdict[t] = v;
    observations[t] = no;
}

template <class T>
int regrow(T** p, size_t count) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    ORB_HIP_CHECK(hipMalloc((void**)p, sizeof(T) * std::max(count, (size_t)1)));
    return 0;
}

}  // namespace

Map::~Map() {
    (void)hipDeviceSynchronize();   // queries run on the matchers' streams as well
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    if (ev_done_) (void)hipEventDestroy(ev_done_);
    void* bufs[] = {d_slots_, d_nb_, d_order_, d_child_, d_id2slot_, d_mp_, d_obs_, d_pt_list_, d_pt_start_,
                    d_pt_cursor_, d_work_, d_scr_, d_counts_, d_q_, d_oct_, d_flags_, d_pt_obs_, d_nobs_,
                    d_cull_scr_, d_dead_, d_cull_io_};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (s_) (void)hipStreamDestroy(s_);
}

int Map::init(int slots, int cells, int points) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -4;
    ORB_HIP_CHECK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
    for (auto& e : ev_) ORB_HIP_CHECK(hipEventCreate(&e));
    ORB_HIP_CHECK(hipEventCreateWithFlags(&ev_done_, hipEventDisableTiming));
    slot_cap_ = std::max(slots, 1);
    pool_cap_ = dev_pool_cap_ = std::max(cells, 1);
    pt_cap_ = std::max(points, 1);
    if (int e = regrow(&d_slots_, (size_t)slot_cap_)) return e;
    if (int e = regrow(&d_nb_, (size_t)slot_cap_)) return e;
    if (int e = regrow(&d_order_, (size_t)slot_cap_)) return e;
    if (int e = regrow(&d_mp_, (size_t)dev_pool_cap_)) return e;
    if (int e = regrow(&d_obs_, (size_t)dev_pool_cap_)) return e;
    if (int e = regrow(&d_pt_list_, (size_t)dev_pool_cap_)) return e;
    if (int e = regrow(&d_pt_start_, (size_t)pt_cap_ + 1)) return e;
    if (int e = regrow(&d_pt_cursor_, (size_t)pt_cap_ + 1)) return e;
    h_mp_.assign((size_t)pool_cap_, -1);
    h_obs_.assign((size_t)pool_cap_, 0);
    h_oct_.assign((size_t)pool_cap_, 0);
    h_flags_.assign((size_t)pool_cap_, 0);
    return 0;
}

// ---------------------------------------------------------------- host mirror

void Map::mark_row(int slot) {
    index_dirty_ = true;
    if (row_dirty_[slot]) return;
    row_dirty_[slot] = 1;
    dirty_rows_.push_back(slot);
}

bool Map::row_holds(int slot, int32_t mp, int except_idx) const {
    auto it = held_.find(mp);
    if (it == held_.end()) return false;
    for (uint32_t c : it->second)
        if ((int)(c / kMapMaxRow) == slot && (int)(c % kMapMaxRow) != except_idx) return true;
    return false;
}

void Map::set_cell(int slot, int idx, int32_t mp, uint8_t obs) {
    const size_t at = (size_t)slots_[slot].off + idx;
    const uint32_t code = (uint32_t)slot * kMapMaxRow + (uint32_t)idx;
    const int32_t old = h_mp_[at];
    if (old >= 0 && h_obs_[at]) n_observed_--;
    if (old >= 0 && old != mp) {
        auto it = held_.find(old);
        if (it != held_.end()) {
            auto& v = it->second;
            for (size_t k = 0; k < v.size(); k++)
                if (v[k] == code) {
                    v[k] = v.back();
                    v.pop_back();
                    break;
                }
            if (v.empty()) held_.erase(it);
        }
    }
    if (mp >= 0 && old != mp) held_[mp].push_back(code);
    h_mp_[at] = mp;
    h_obs_[at] = mp >= 0 ? (obs != 0) : 0;
    if (mp >= 0 && h_obs_[at]) n_observed_++;
    if (mp >= npts_) npts_ = mp + 1;
    mark_row(slot);
}

// Move the live rows of the host pools into pools of new_cap cells, holes squeezed out; the
// device pools follow at the next query (every row is uploaded again).
int Map::repack(long long new_cap) {
    if (new_cap > 0x7fffffffLL) return -3;
    std::vector<int32_t> nm((size_t)new_cap, -1);
    std::vector<uint8_t> no((size_t)new_cap, 0), nk((size_t)new_cap, 0), nf((size_t)new_cap, 0);
    long long used = 0;
    for (size_t sl = 0; sl < slots_.size(); sl++) {
        MapSlotDev& S = slots_[sl];
        if (!S.live) continue;
        std::memcpy(nm.data() + used, h_mp_.data() + S.off, 4 * (size_t)S.n);
        std::memcpy(no.data() + used, h_obs_.data() + S.off, (size_t)S.n);
        std::memcpy(nk.data() + used, h_oct_.data() + S.off, (size_t)S.n);
        std::memcpy(nf.data() + used, h_flags_.data() + S.off, (size_t)S.n);
        S.off = (int32_t)used;
        used += S.n;
    }
    h_mp_.swap(nm);
    h_obs_.swap(no);
    h_oct_.swap(nk);
    h_flags_.swap(nf);
    pool_cap_ = new_cap;
    pool_used_ = used;
    all_rows_dirty_ = meta_dirty_ = index_dirty_ = true;
    return 0;
}

int Map::add_keyframe(int32_t id, int N, const int32_t* mp, const uint8_t* observed) {
    if (live_cells_ + N > 0x7fffffffLL) return -3;
    if (pool_used_ + N > pool_cap_) {
        long long cap = pool_cap_;
        while (live_cells_ + N > cap) cap *= 2;
        if (cap > 0x7fffffffLL) cap = 0x7fffffffLL;
        if (int e = repack(cap)) return e;
    }
    int sl;
    if (!free_.empty()) {
        sl = free_.back();
        free_.pop_back();
    } else {
        sl = (int)slots_.size();
        slots_.push_back(MapSlotDev{});
        nb_.push_back(Nb{});
        row_dirty_.push_back(0);
    }
    slots_[sl] = MapSlotDev{id, (int32_t)pool_used_, N, 1};
    nb_[sl] = Nb{};
    slot_of_[id] = sl;
    for (int i = 0; i < N; i++) {   // the span may hold an erased row's cells
        h_mp_[(size_t)pool_used_ + i] = -1;
        h_obs_[(size_t)pool_used_ + i] = 0;
        h_oct_[(size_t)pool_used_ + i] = 0;   // keys never set: octave 0, monocular, not far
        h_flags_[(size_t)pool_used_ + i] = 0;
    }
    pool_used_ += N;
    live_cells_ += N;
    if (id >= nid_) nid_ = id + 1;
    for (int i = 0; i < N; i++)
        if (mp[i] >= 0) set_cell(sl, i, mp[i], observed ? observed[i] : 1);
    mark_row(sl);
    meta_dirty_ = true;
    return 0;
}

int Map::set_matches(int32_t id, int count, const int32_t* slot, const int32_t* mp, const uint8_t* observed) {
    const int sl = slot_of(id);
    if (sl < 0) return -1;
    for (int k = 0; k < count; k++) {
        if (slot[k] < 0 || slot[k] >= slots_[sl].n) return -1;
        if (mp[k] >= 0 && row_holds(sl, mp[k], slot[k])) return -1;
    }
    for (int k = 0; k < count; k++) set_cell(sl, slot[k], mp[k] < 0 ? -1 : mp[k], observed ? observed[k] : 1);
    return 0;
}

int Map::erase_point(int32_t mp) {
    auto it = held_.find(mp);
    if (it == held_.end()) return 0;
    const std::vector<uint32_t> cells = it->second;
    for (uint32_t c : cells) set_cell((int)(c / kMapMaxRow), (int)(c % kMapMaxRow), -1, 0);
    return 0;
}

int Map::replace_point(int32_t mp, int32_t by) {
    if (mp == by) return 0;   // MapPoint.cc: Replace(this) returns
    auto it = held_.find(mp);
    if (it == held_.end()) return 0;
    const std::vector<uint32_t> cells = it->second;
    for (uint32_t c : cells) {
        const int sl = (int)(c / kMapMaxRow), idx = (int)(c % kMapMaxRow);
        const bool obs = h_obs_[(size_t)slots_[sl].off + idx] != 0;
        if (obs && !row_holds(sl, by, -1)) set_cell(sl, idx, by, 1);
        else set_cell(sl, idx, -1, 0);
    }
    return 0;
}

int Map::erase_keyframe(int32_t id) {
    auto it = slot_of_.find(id);
    if (it == slot_of_.end()) return 0;
    const int sl = it->second;
    for (int i = 0; i < slots_[sl].n; i++)
        if (h_mp_[(size_t)slots_[sl].off + i] >= 0) set_cell(sl, i, -1, 0);
    slots_[sl].live = 0;
    live_cells_ -= slots_[sl].n;
    slots_[sl].n = 0;
    nb_[sl] = Nb{};
    free_.push_back(sl);
    slot_of_.erase(it);
    meta_dirty_ = index_dirty_ = true;
    if (pool_used_ - live_cells_ > live_cells_ && pool_used_ > 0) return repack(pool_cap_);
    return 0;
}

int Map::set_neighbours(int32_t id, int n10, const int32_t* ids10, int32_t parent, int nchild,
                        const int32_t* children) {
    const int sl = slot_of(id);
    if (sl < 0) return -1;
    Nb& N = nb_[sl];
    N.ncov = n10;
    for (int k = 0; k < n10; k++) N.cov[k] = ids10[k];
    N.parent = parent;
    N.children.assign(children, children + nchild);
    std::sort(N.children.begin(), N.children.end());   // id order for the std::set's address order
    meta_dirty_ = true;
    return 0;
}

int Map::set_keys(int32_t id, int N, const uint8_t* octave, const float* uRight, const float* depth, float thDepth) {
    const int sl = slot_of(id);
    if (sl < 0 || N != slots_[sl].n) return -1;
    const size_t off = (size_t)slots_[sl].off;
    for (int i = 0; i < N; i++) {
        h_oct_[off + i] = octave[i];
        uint8_t f = 0;
        if (uRight && uRight[i] >= 0.f) f |= kMapKeyStereo;
        if (depth && (depth[i] > thDepth || depth[i] < 0.f)) f |= kMapKeyFar;
        h_flags_[off + i] = f;
    }
    cull_dirty_ = true;
    return 0;
}

int Map::clear() {
    slots_.clear();
    nb_.clear();
    free_.clear();
    slot_of_.clear();
    held_.clear();
    row_dirty_.clear();
    dirty_rows_.clear();
    pool_used_ = live_cells_ = n_observed_ = 0;
    all_rows_dirty_ = meta_dirty_ = index_dirty_ = true;
    return 0;
}

// ---------------------------------------------------------------- device state

int Map::drain() {
    if (ev_recorded_) ORB_HIP_CHECK(hipEventSynchronize(ev_done_));
    return 0;
}

// Stream `s` starts a query: behind the last query of any other stream (the tables, the index
// and the work area are the handle's).
int Map::join(hipStream_t s) {
    if (ev_recorded_ && last_stream_ != s) ORB_HIP_CHECK(hipStreamWaitEvent(s, ev_done_, 0));
    return 0;
}

int Map::leave(hipStream_t s) {
    ORB_HIP_CHECK(hipEventRecord(ev_done_, s));
    ev_recorded_ = true;
    last_stream_ = s;
    return 0;
}

// Upload what the mutations since the last query changed and rebuild the inverse index, on `s`.
// The sources are the pageable host mirror, so the stream is waited for before returning.
int Map::sync_device(hipStream_t s) {
    timed_rebuild_ = false;
    if (!all_rows_dirty_ && !meta_dirty_ && !index_dirty_ && dirty_rows_.empty()) return 0;
    cull_dirty_ = true;   // the cell index and nObs follow at the next culling call
    const int nslots = (int)slots_.size();
    // growth: nothing queued may still read the old buffers
    if (nslots > slot_cap_ || pool_cap_ > dev_pool_cap_ || npts_ > pt_cap_ || nid_ > id_cap_) {
        if (int e = drain()) return e;
        ORB_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (nslots > slot_cap_) {
        int cap = slot_cap_;
        while (nslots > cap) cap *= 2;
        if (int e = regrow(&d_slots_, (size_t)cap)) return e;
        if (int e = regrow(&d_nb_, (size_t)cap)) return e;
        if (int e = regrow(&d_order_, (size_t)cap)) return e;
        slot_cap_ = cap;
        meta_dirty_ = true;
    }
    if (pool_cap_ > dev_pool_cap_) {
        if (int e = regrow(&d_mp_, (size_t)pool_cap_)) return e;
        if (int e = regrow(&d_obs_, (size_t)pool_cap_)) return e;
        if (int e = regrow(&d_pt_list_, (size_t)pool_cap_)) return e;
        dev_pool_cap_ = pool_cap_;
        all_rows_dirty_ = true;
    }
    if (npts_ > pt_cap_) {
        int cap = pt_cap_;
        while (npts_ > cap) cap *= 2;
        if (int e = regrow(&d_pt_start_, (size_t)cap + 1)) return e;
        if (int e = regrow(&d_pt_cursor_, (size_t)cap + 1)) return e;
        pt_cap_ = cap;
    }
    if (nid_ > id_cap_) {
        int cap = std::max(id_cap_, 1024);
        while (nid_ > cap) cap *= 2;
        if (int e = regrow(&d_id2slot_, (size_t)cap)) return e;
        id_cap_ = cap;
        meta_dirty_ = true;
    }
    if (timing_) ORB_HIP_CHECK(hipEventRecord(ev_[0], s));
    if (all_rows_dirty_) {
        if (pool_used_ > 0) {
            ORB_HIP_CHECK(hipMemcpyAsync(d_mp_, h_mp_.data(), 4 * (size_t)pool_used_, hipMemcpyHostToDevice, s));
            ORB_HIP_CHECK(hipMemcpyAsync(d_obs_, h_obs_.data(), (size_t)pool_used_, hipMemcpyHostToDevice, s));
        }
    } else {
        for (int sl : dirty_rows_) {
            const MapSlotDev& S = slots_[sl];
            if (!S.live || S.n == 0) continue;
            ORB_HIP_CHECK(hipMemcpyAsync(d_mp_ + S.off, h_mp_.data() + S.off, 4 * (size_t)S.n, hipMemcpyHostToDevice, s));
            ORB_HIP_CHECK(hipMemcpyAsync(d_obs_ + S.off, h_obs_.data() + S.off, (size_t)S.n, hipMemcpyHostToDevice, s));
        }
    }
    for (int sl : dirty_rows_)
        if (sl < (int)row_dirty_.size()) row_dirty_[sl] = 0;
    dirty_rows_.clear();
    all_rows_dirty_ = false;
    std::vector<int32_t> order, id2slot, child;
    std::vector<MapNbDev> nbd;
    if (meta_dirty_) {
        order.reserve(slot_of_.size());
        for (const auto& kv : slot_of_) order.push_back(kv.second);
        std::sort(order.begin(), order.end(), [&](int a, int b) { return slots_[a].id < slots_[b].id; });
        id2slot.assign((size_t)std::max(nid_, 1), -1);
        for (const auto& kv : slot_of_) id2slot[kv.first] = kv.second;
        nbd.resize((size_t)std::max(nslots, 1));
        for (int sl = 0; sl < nslots; sl++) {
            MapNbDev& D = nbd[sl];
            std::memset(&D, 0, sizeof(D));
            D.parent = -1;
            if (!slots_[sl].live) continue;
            const Nb& N = nb_[sl];
            D.ncov = N.ncov;
            for (int k = 0; k < N.ncov; k++) D.cov[k] = N.cov[k];
            D.parent = N.parent;
            D.child_off = (int32_t)child.size();
            D.nchild = (int32_t)N.children.size();
            child.insert(child.end(), N.children.begin(), N.children.end());
        }
        if ((int)child.size() > child_cap_) {
            if (int e = drain()) return e;
            ORB_HIP_CHECK(hipStreamSynchronize(s));
            const int cap = std::max((int)child.size() * 2, 1024);
            if (int e = regrow(&d_child_, (size_t)cap)) return e;
            child_cap_ = cap;
        }
        if (nslots > 0) {
            ORB_HIP_CHECK(hipMemcpyAsync(d_slots_, slots_.data(), sizeof(MapSlotDev) * (size_t)nslots, hipMemcpyHostToDevice, s));
            ORB_HIP_CHECK(hipMemcpyAsync(d_nb_, nbd.data(), sizeof(MapNbDev) * (size_t)nslots, hipMemcpyHostToDevice, s));
        }
        if (!order.empty())
            ORB_HIP_CHECK(hipMemcpyAsync(d_order_, order.data(), 4 * order.size(), hipMemcpyHostToDevice, s));
        if (nid_ > 0)
            ORB_HIP_CHECK(hipMemcpyAsync(d_id2slot_, id2slot.data(), 4 * (size_t)nid_, hipMemcpyHostToDevice, s));
        if (!child.empty())
            ORB_HIP_CHECK(hipMemcpyAsync(d_child_, child.data(), 4 * child.size(), hipMemcpyHostToDevice, s));
        n_live_dev_ = (int)order.size();
        meta_dirty_ = false;
    }
    // the inverse index: count, exclusive scan, fill
    ORB_HIP_CHECK(hipMemsetAsync(d_pt_start_, 0, 4 * ((size_t)npts_ + 1), s));
    if (n_live_dev_ > 0 && npts_ > 0)
        hipLaunchKernelGGL(k_map_csr_count, dim3(n_live_dev_), dim3(MT), 0, s, d_slots_, d_order_, d_mp_, d_obs_, npts_,
                           d_pt_start_);
    hipLaunchKernelGGL(k_map_csr_scan, dim3(1), dim3(MSCAN), 0, s, (int)npts_, d_pt_start_, d_pt_cursor_);
    if (n_live_dev_ > 0 && npts_ > 0)
        hipLaunchKernelGGL(k_map_csr_fill, dim3(n_live_dev_), dim3(MT), 0, s, d_slots_, d_order_, d_mp_, d_obs_, npts_,
                           d_pt_cursor_, d_pt_list_);
    ORB_HIP_CHECK(hipGetLastError());
    if (timing_) {
        ORB_HIP_CHECK(hipEventRecord(ev_[1], s));
        timed_rebuild_ = true;
    }
    index_dirty_ = false;
    ORB_HIP_CHECK(hipStreamSynchronize(s));   // the host vectors above and the mirror are pageable
    return 0;
}

// cnt | kfslot | rowcnt | rowoff for `chunk` frames, and the first-occurrence scratch
int Map::reserve_work(int chunk) {
    const int nslots = std::max((int)slots_.size(), 1);
    const int nscr = std::max(npts_, 1);
    if (chunk <= work_chunk_ && nslots <= work_stride_ && nscr <= scr_stride_) return 0;
    if (int e = drain()) return e;
    const int ch = std::max(chunk, work_chunk_);
    int st = std::max(work_stride_, 256), sc = std::max(scr_stride_, 1024);
    while (nslots > st) st *= 2;
    while (nscr > sc) sc *= 2;
    ORB_HIP_CHECK(hipDeviceSynchronize());
    if (int e = regrow(&d_work_, 4 * (size_t)ch * st)) return e;
    if (int e = regrow(&d_scr_, (size_t)ch * sc)) return e;
    if (int e = regrow(&d_counts_, (size_t)ch)) return e;
    if (int e = regrow(&d_q_, (size_t)ch)) return e;
    hipLaunchKernelGGL(k_map_fill, dim3(1024), dim3(MT), 0, s_, d_scr_, (size_t)ch * sc, kIdle);
    ORB_HIP_CHECK(hipGetLastError());
    ORB_HIP_CHECK(hipStreamSynchronize(s_));
    work_chunk_ = ch;
    work_stride_ = st;
    scr_stride_ = sc;
    return 0;
}

int Map::vote_rows(int count, const int32_t* ids) {
    const int nslots = (int)slots_.size();
    h_votes_.assign((size_t)count * std::max(nslots, 1), 0);
    if (count <= 0 || nslots == 0) return 0;
    hipStream_t s = s_;
    if (int e = join(s)) return e;
    if (int e = sync_device(s)) return e;
    const int chunk = std::max(1, std::min(count, chunk_ > 0 ? chunk_ : kMapDefaultChunk));
    if (int e = reserve_work(chunk)) return e;
    const int lds_max = lds_slots_ >= 0 ? std::min(lds_slots_, kMapLdsSlots) : kMapLdsSlots;
    const bool lds = nslots <= lds_max;
    std::vector<MapQueryDev> q((size_t)chunk);
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int nc = std::min(chunk, count - c0);
        for (int i = 0; i < nc; i++) {
            const int sl = slot_of(ids[c0 + i]);
            const MapSlotDev& S = slots_[sl];
            q[i] = MapQueryDev{d_mp_ + S.off, nullptr, S.n, 0, sl, 0};
        }
        ORB_HIP_CHECK(hipMemcpyAsync(d_q_, q.data(), sizeof(MapQueryDev) * (size_t)nc, hipMemcpyHostToDevice, s));
        if (lds) {
            hipLaunchKernelGGL(k_map_vote<true>, dim3(nc), dim3(MV), 4 * (size_t)nslots, s, (const uint8_t*)d_q_,
                               sizeof(MapQueryDev), d_pt_start_, d_pt_list_, (int)npts_, nslots, work_stride_, d_work_);
        } else {
            ORB_HIP_CHECK(hipMemsetAsync(d_work_, 0, 4 * (size_t)nc * work_stride_, s));
            hipLaunchKernelGGL(k_map_vote<false>, dim3(nc), dim3(MV), 0, s, (const uint8_t*)d_q_, sizeof(MapQueryDev),
                               d_pt_start_, d_pt_list_, (int)npts_, nslots, work_stride_, d_work_);
        }
        ORB_HIP_CHECK(hipGetLastError());
        ORB_HIP_CHECK(hipMemcpy2DAsync(h_votes_.data() + (size_t)c0 * nslots, 4 * (size_t)nslots, d_work_,
                                       4 * (size_t)work_stride_, 4 * (size_t)nslots, (size_t)nc,
                                       hipMemcpyDeviceToHost, s));
        ORB_HIP_CHECK(hipStreamSynchronize(s));   // q and the work area are reused by the next chunk
    }
    return leave(s);
}

int Map::update_local(hipStream_t s, int count, const MapLocalDev* d_frames, const MapLocalDev* h_frames) {
    timed_ = false;
    if (count <= 0) return 0;
    if (int e = join(s)) return e;
    if (int e = sync_device(s)) return e;
    const int nslots = (int)slots_.size();
    const int nscr_need = std::max(npts_, 1);
    int chunk = chunk_ > 0 ? chunk_ : kMapDefaultChunk;
    chunk = std::min(chunk, (int)std::max((size_t)1, kMapScratchBytes / (4 * (size_t)std::max(nscr_need, scr_stride_))));
    chunk = std::max(1, std::min(chunk, count));
    if (int e = reserve_work(chunk)) return e;
    const int stride = work_stride_, nscr = scr_stride_;
    const size_t cells = (size_t)work_chunk_ * stride;
    int32_t* d_cnt = d_work_;
    int32_t* d_kfslot = d_work_ + cells;
    int32_t* d_rowcnt = d_work_ + 2 * cells;
    int32_t* d_rowoff = d_work_ + 3 * cells;
    const int lds_max = lds_slots_ >= 0 ? std::min(lds_slots_, kMapLdsSlots) : kMapLdsSlots;
    const bool lds = nslots <= lds_max;
    const int n_live = n_live_dev_;
    for (int c0 = 0; c0 < count; c0 += chunk) {
        const int nc = std::min(chunk, count - c0);
        const MapLocalDev* F = d_frames + c0;
        int maxN = 1, maxP = 1;
        for (int i = 0; i < nc; i++) {
            maxN = std::max(maxN, h_frames[c0 + i].q.n);
            maxP = std::max(maxP, h_frames[c0 + i].pt_cap);
        }
        const bool tm = timing_ && c0 + nc >= count;
        if (tm) ORB_HIP_CHECK(hipEventRecord(ev_[2], s));
        if (lds) {
            hipLaunchKernelGGL(k_map_vote<true>, dim3(nc), dim3(MV), 4 * (size_t)std::max(nslots, 1), s,
                               (const uint8_t*)F, sizeof(MapLocalDev), d_pt_start_, d_pt_list_, (int)npts_, nslots,
                               stride, d_cnt);
        } else {
            ORB_HIP_CHECK(hipMemsetAsync(d_cnt, 0, 4 * (size_t)nc * stride, s));
            hipLaunchKernelGGL(k_map_vote<false>, dim3(nc), dim3(MV), 0, s, (const uint8_t*)F, sizeof(MapLocalDev),
                               d_pt_start_, d_pt_list_, (int)npts_, nslots, stride, d_cnt);
        }
        if (tm) ORB_HIP_CHECK(hipEventRecord(ev_[3], s));
        hipLaunchKernelGGL(k_map_select, dim3(nc), dim3(MT), 0, s, F, d_order_, n_live, d_slots_, d_nb_, d_child_,
                           d_id2slot_, (int)nid_, stride, d_cnt, d_kfslot);
        if (tm) ORB_HIP_CHECK(hipEventRecord(ev_[4], s));
        if (n_live > 0) {
            const dim3 g((unsigned)n_live, (unsigned)nc);
            hipLaunchKernelGGL(k_map_pt_min, g, dim3(MT), 0, s, F, d_slots_, d_mp_, stride, d_kfslot, nscr, d_scr_);
            hipLaunchKernelGGL(k_map_pt_count, g, dim3(MT), 0, s, F, d_slots_, d_mp_, stride, d_kfslot, nscr, d_scr_,
                               d_rowcnt);
            hipLaunchKernelGGL(k_map_pt_scan, dim3(nc), dim3(MT), 0, s, F, stride, d_rowcnt, d_rowoff);
            hipLaunchKernelGGL(k_map_pt_write, g, dim3(MT), 0, s, F, d_slots_, d_mp_, stride, d_kfslot, d_rowoff, nscr,
                               d_scr_);
        }
        if (tm) ORB_HIP_CHECK(hipEventRecord(ev_[5], s));
        hipLaunchKernelGGL(k_map_remap, dim3((unsigned)((std::max(maxN, maxP) + MT - 1) / MT), (unsigned)nc), dim3(MT), 0,
                           s, F, nscr, d_scr_);
        if (tm) ORB_HIP_CHECK(hipEventRecord(ev_[6], s));
        if (n_live > 0)
            hipLaunchKernelGGL(k_map_restore, dim3((unsigned)n_live, (unsigned)nc), dim3(MT), 0, s, F, d_slots_, d_mp_,
                               stride, d_kfslot, nscr, d_scr_);
        ORB_HIP_CHECK(hipGetLastError());
        if (tm) timed_ = true;
    }
    return leave(s);
}

int Map::timings(float* ms5) {
    if (!timed_) return -1;
    ORB_HIP_CHECK(hipEventSynchronize(ev_[6]));
    ms5[0] = -1.f;
    if (timed_rebuild_) ORB_HIP_CHECK(hipEventElapsedTime(&ms5[0], ev_[0], ev_[1]));
    for (int i = 0; i < 4; i++) ORB_HIP_CHECK(hipEventElapsedTime(&ms5[1 + i], ev_[2 + i], ev_[3 + i]));
    return 0;
}

// ---------------------------------------------------------------- culling

// After sync_device: the key attributes, the cell index and nObs, when a mutation or
// Map_SetKeyFrameKeys came since the last culling call.  UpdateLocalMap and UpdateConnections
// never pay for them.
int Map::sync_cull(hipStream_t s) {
    const int nslots = (int)slots_.size();
    if (dev_pool_cap_ > cull_pool_cap_ || pt_cap_ > cull_pt_cap_ || slot_cap_ > cull_slot_cap_) {
        if (int e = drain()) return e;
        ORB_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (dev_pool_cap_ > cull_pool_cap_) {
        if (int e = regrow(&d_oct_, (size_t)dev_pool_cap_)) return e;
        if (int e = regrow(&d_flags_, (size_t)dev_pool_cap_)) return e;
        if (int e = regrow(&d_pt_obs_, (size_t)dev_pool_cap_)) return e;
        cull_pool_cap_ = dev_pool_cap_;
        cull_dirty_ = true;
    }
    if (pt_cap_ > cull_pt_cap_) {
        if (int e = regrow(&d_nobs_, (size_t)pt_cap_ + 1)) return e;
        if (int e = regrow(&d_cull_scr_, (size_t)pt_cap_ + 1)) return e;
        cull_pt_cap_ = pt_cap_;
        cull_dirty_ = true;
    }
    if (slot_cap_ > cull_slot_cap_) {
        if (int e = regrow(&d_dead_, (size_t)slot_cap_)) return e;
        cull_slot_cap_ = slot_cap_;
    }
    if (!cull_dirty_) return 0;
    if (pool_used_ > 0) {
        ORB_HIP_CHECK(hipMemcpyAsync(d_oct_, h_oct_.data(), (size_t)pool_used_, hipMemcpyHostToDevice, s));
        ORB_HIP_CHECK(hipMemcpyAsync(d_flags_, h_flags_.data(), (size_t)pool_used_, hipMemcpyHostToDevice, s));
    }
    ORB_HIP_CHECK(hipMemsetAsync(d_nobs_, 0, 4 * ((size_t)npts_ + 1), s));
    if (n_live_dev_ > 0 && npts_ > 0 && nslots > 0) {
        ORB_HIP_CHECK(hipMemcpyAsync(d_pt_cursor_, d_pt_start_, 4 * ((size_t)npts_ + 1), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(k_cull_index, dim3(n_live_dev_), dim3(MT), 0, s, d_slots_, d_order_, d_mp_, d_obs_, d_flags_,
                           (int)npts_, d_pt_cursor_, d_pt_obs_, d_nobs_);
        ORB_HIP_CHECK(hipGetLastError());
    }
    ORB_HIP_CHECK(hipStreamSynchronize(s));   // the mirror is pageable
    cull_dirty_ = false;
    return 0;
}

namespace {
size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }
}  // namespace

int Map::cull_keyframes(MapKfCull& c) {
    hipStream_t s = s_;
    const int n = c.n;
    c.n_bad = 0;
    if (n == 0) return 0;
    std::vector<int32_t> cand_slot((size_t)n);
    bool any = false;
    for (int i = 0; i < n; i++) {
        cand_slot[i] = c.cand[i] == 0 ? -1 : slot_of(c.cand[i]);   // LocalMapping.cc: mnId == 0 is never culled
        any = any || cand_slot[i] >= 0;
    }
    if (!any) {
        for (int i = 0; i < n; i++) {
            c.nMPs[i] = c.nRedundant[i] = 0;
            c.verdict[i] = 3;
        }
        return 0;
    }
    if (int e = join(s)) return e;
    if (int e = sync_device(s)) return e;
    if (int e = sync_cull(s)) return e;
    const int nslots = (int)slots_.size();
    const int cap_dev = std::min(c.cap_bad, (int)npts_);   // no more points than there are can go bad
    // in: cand_slot | not_erase | bad;  out: nmps | nred | verdict | n_bad | bad_mp
    const size_t o_ne = al256(4 * (size_t)n), o_bad = o_ne + al256((size_t)n);
    const size_t in_bytes = o_bad + al256((size_t)c.nbad);
    const size_t o_out = in_bytes, o_nred = o_out + al256(4 * (size_t)n), o_ver = o_nred + al256(4 * (size_t)n);
    const size_t o_nb = o_ver + al256(4 * (size_t)n), o_bmp = o_nb + 256;
    const size_t total = o_bmp + al256(4 * (size_t)cap_dev);
    if (total > cull_io_cap_) {
        if (int e = drain()) return e;
        ORB_HIP_CHECK(hipStreamSynchronize(s));
        if (int e = regrow(&d_cull_io_, total * 2)) return e;
        cull_io_cap_ = total * 2;
    }
    std::vector<uint8_t> io(total, 0);
    std::memcpy(io.data(), cand_slot.data(), 4 * (size_t)n);
    if (c.not_erase) std::memcpy(io.data() + o_ne, c.not_erase, (size_t)n);
    if (c.bad && c.nbad > 0) std::memcpy(io.data() + o_bad, c.bad, (size_t)c.nbad);
    ORB_HIP_CHECK(hipMemcpyAsync(d_cull_io_, io.data(), in_bytes, hipMemcpyHostToDevice, s));
    ORB_HIP_CHECK(hipMemsetAsync(d_cull_scr_, 0, 4 * ((size_t)npts_ + 1), s));
    ORB_HIP_CHECK(hipMemsetAsync(d_dead_, 0, (size_t)std::max(nslots, 1), s));
    CullDev C;
    C.slots = d_slots_; C.mp = d_mp_; C.obs = d_obs_; C.oct = d_oct_; C.flags = d_flags_;
    C.pt_start = d_pt_start_; C.pt_obs = d_pt_obs_; C.nobs = d_nobs_; C.scr = d_cull_scr_; C.dead = d_dead_;
    C.bad = (c.bad && c.nbad > 0) ? d_cull_io_ + o_bad : nullptr;
    C.nbad = c.nbad;
    C.monocular = c.monocular != 0;
    const int32_t* d_cand = (const int32_t*)d_cull_io_;
    int32_t* d_nmps = (int32_t*)(d_cull_io_ + o_out);
    int32_t* d_nred = (int32_t*)(d_cull_io_ + o_nred);
    int32_t* d_ver = (int32_t*)(d_cull_io_ + o_ver);
    int32_t* d_nb = (int32_t*)(d_cull_io_ + o_nb);
    int32_t* d_bmp = (int32_t*)(d_cull_io_ + o_bmp);
    hipLaunchKernelGGL(k_cull_count, dim3(n), dim3(MT), 0, s, C, d_cand, d_nmps, d_nred);
    hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(MT), 0, s, C, n, d_cand,
                       c.not_erase ? (const uint8_t*)(d_cull_io_ + o_ne) : nullptr, cap_dev, d_nmps, d_nred, d_ver, d_bmp,
                       d_nb);
    ORB_HIP_CHECK(hipGetLastError());
    ORB_HIP_CHECK(hipMemcpyAsync(io.data() + o_out, d_cull_io_ + o_out, total - o_out, hipMemcpyDeviceToHost, s));
    ORB_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(c.nMPs, io.data() + o_out, 4 * (size_t)n);
    std::memcpy(c.nRedundant, io.data() + o_nred, 4 * (size_t)n);
    std::memcpy(c.verdict, io.data() + o_ver, 4 * (size_t)n);
    std::memcpy(&c.n_bad, io.data() + o_nb, 4);
    const int nw = std::min(c.n_bad, cap_dev);
    if (nw > 0) std::memcpy(c.bad_mp, io.data() + o_bmp, 4 * (size_t)nw);
    if (int e = leave(s)) return e;
    return c.n_bad > c.cap_bad ? -3 : 0;
}

int Map::cull_points(const MapPtCull& c) {
    hipStream_t s = s_;
    const int n = c.n;
    if (n == 0) return 0;
    if (int e = join(s)) return e;
    if (int e = sync_device(s)) return e;
    if (int e = sync_cull(s)) return e;
    // in: mp | first_kf | found | visible | bad;  out: verdict | observations
    const size_t w = al256(4 * (size_t)n);
    const size_t o_bad = 4 * w, in_bytes = o_bad + al256((size_t)c.nbad), o_out = in_bytes, total = o_out + 2 * w;
    if (total > cull_io_cap_) {
        if (int e = drain()) return e;
        ORB_HIP_CHECK(hipStreamSynchronize(s));
        if (int e = regrow(&d_cull_io_, total * 2)) return e;
        cull_io_cap_ = total * 2;
    }
    std::vector<uint8_t> io(total, 0);
    const int32_t* src[4] = {c.mp, c.first_kf, c.found, c.visible};
    for (int k = 0; k < 4; k++) std::memcpy(io.data() + k * w, src[k], 4 * (size_t)n);
    if (c.bad && c.nbad > 0) std::memcpy(io.data() + o_bad, c.bad, (size_t)c.nbad);
    ORB_HIP_CHECK(hipMemcpyAsync(d_cull_io_, io.data(), in_bytes, hipMemcpyHostToDevice, s));
    auto at = [&](size_t o) { return (int32_t*)(d_cull_io_ + o); };
    hipLaunchKernelGGL(k_cull_points, dim3((unsigned)((n + MT - 1) / MT)), dim3(MT), 0, s, n, at(0), at(w), at(2 * w),
                       at(3 * w), (c.bad && c.nbad > 0) ? (const uint8_t*)(d_cull_io_ + o_bad) : nullptr, c.nbad, d_nobs_,
                       (int)npts_, (int)c.cur_kf, c.monocular ? 2 : 3, at(o_out), at(o_out + w));
    ORB_HIP_CHECK(hipGetLastError());
    ORB_HIP_CHECK(hipMemcpyAsync(io.data() + o_out, d_cull_io_ + o_out, 2 * w, hipMemcpyDeviceToHost, s));
    ORB_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(c.verdict, io.data() + o_out, 4 * (size_t)n);
    if (c.observations) std::memcpy(c.observations, io.data() + o_out + w, 4 * (size_t)n);
    return leave(s);
}

int Map::begin_view(hipStream_t s, MapView& v) {
    if (int e = join(s)) return e;
    if (int e = sync_device(s)) return e;
    if (int e = sync_cull(s)) return e;
    v.slots = d_slots_;
    v.mp = d_mp_;
    v.obs = d_obs_;
    v.oct = d_oct_;
    v.pt_start = d_pt_start_;
    v.pt_obs = d_pt_obs_;
    v.npts = n_live_dev_ > 0 ? npts_ : 0;   // without a live row the index was never filled
    return 0;
}

// Three-colour depth-first search over the children lists, without recursion (a chain may be as
// long as the map).  Children that are not live are skipped, as every reader skips them.
bool Map::children_cyclic() const {
    std::vector<uint8_t> colour(slots_.size(), 0);   // 0 new, 1 on the path, 2 done
    std::vector<std::pair<int, size_t>> path;
    for (const auto& kv : slot_of_) {
        if (colour[kv.second]) continue;
        colour[kv.second] = 1;
        path.emplace_back(kv.second, 0);
        while (!path.empty()) {
            const int sl = path.back().first;
            const std::vector<int32_t>& ch = nb_[sl].children;
            if (path.back().second == ch.size()) {
                colour[sl] = 2;
                path.pop_back();
                continue;
            }
            const int c = slot_of(ch[path.back().second++]);
            if (c < 0 || colour[c] == 2) continue;
            if (colour[c] == 1) return true;
            colour[c] = 1;
            path.emplace_back(c, 0);
        }
    }
    return false;
}

}  // namespace orbgpu
