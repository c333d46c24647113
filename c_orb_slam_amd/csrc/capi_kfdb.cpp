// capi_kfdb.cpp -- extern "C" KeyFrameDatabase_* (include/orbslam_gpu.h), reference
// include/KeyFrameDatabase.h and src/KeyFrameDatabase.cc.
// Host pointers only.  The scan over the stored BowVectors (shared words, maxCommonWords, the
// scored subset and its L1 scores) runs on the device (kfdb.hip); a query downloads the scored
// subset once and the list logic over it -- the order of lKFsSharingWords, the accumulation over
// the covisibles, retention and de-duplication (146-194, 263-306) -- is replayed here in the
// reference's order and float arithmetic.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <limits>
#include <mutex>
#include <new>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/orbslam_gpu.h"
#include "kfdb.hpp"

using orbgpu::KfdbQuery;
using orbgpu::KfdbScored;

struct KeyFrameDatabase_t {
    ORBvocabulary_h voc = nullptr;
    orbgpu::KfDatabase db;
    std::mutex mu;
    // GetBestCovisibilityKeyFrames(10) per keyframe id: the keyframe's property, not the entry's
    std::unordered_map<int32_t, std::vector<int32_t>> covis;
    bool timing = false, timed = false;
    float ms[3] = {};
};

namespace {

constexpr int kDefaultSlots = 1024, kDefaultEntries = 1 << 20;
std::atomic<int> g_init_slots{kDefaultSlots}, g_init_entries{kDefaultEntries};   // orbgpu_unit_set_kfdb_initial_capacity

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

int rc_of(int e) { return e == 0 ? ORB_OK : e == -4 ? ORB_E_NODEVICE : e == -3 ? ORB_E_CAPACITY : ORB_E_HIP; }

// a BowVector as the std::map holds it: strictly ascending words
bool ascending(const uint32_t* w, int n) {
    for (int i = 1; i < n; i++)
        if (w[i] <= w[i - 1]) return false;
    return true;
}

int vocab_words(ORBvocabulary_h voc, int* scoring) {
    int nwords = 0;
    if (ORBvocabulary_info(voc, nullptr, nullptr, scoring, nullptr, nullptr, &nwords) != ORB_OK) return -1;
    return nwords;
}

// shape checks of `count` keyframes as CSR, before the device and the handle
int check_csr(int count, const int32_t* id, const int32_t* start, const uint32_t* word, const double* value) {
    if (count < 0 || (count > 0 && (!id || !start))) return ORB_E_INVALID;
    if (count == 0) return ORB_OK;
    if (start[0] != 0) return ORB_E_INVALID;
    for (int i = 0; i < count; i++) {
        const long long n = (long long)start[i + 1] - start[i];
        if (n < 0 || n > orbgpu::kKfdbMaxWords || id[i] < 0) return ORB_E_INVALID;
    }
    if (start[count] > 0 && (!word || !value)) return ORB_E_INVALID;
    for (int i = 0; i < count; i++)
        if (!ascending(word + start[i], start[i + 1] - start[i])) return ORB_E_INVALID;
    return ORB_OK;
}

int check_query(const orb_kfdb_query* q, const orb_kfdb_result* r, bool loop) {
    if (!q || !r) return ORB_E_INVALID;
    if (q->nq < 0 || q->nq > orbgpu::kKfdbMaxWords || (q->nq > 0 && (!q->word || !q->value))) return ORB_E_INVALID;
    if (!ascending(q->word, q->nq)) return ORB_E_INVALID;
    if (loop && (q->n_exclude < 0 || (q->n_exclude > 0 && !q->exclude))) return ORB_E_INVALID;
    if (r->cap < 0 || (r->cap > 0 && !r->cand) || r->cap_scored < 0) return ORB_E_INVALID;
    return ORB_OK;
}

struct Entry {
    int32_t id, words, first;
    long long seq;
    float score;
};

// KeyFrameDatabase.cc:146-194 (loop) / 263-306 (relocalization) over the scored subset of one query
int finish_query(KeyFrameDatabase_t* h, int qi, const orb_kfdb_query& q, orb_kfdb_result& r, bool loop) {
    const orbgpu::KfdbCounts& c = h->db.counts(qi);
    const KfdbScored* S = h->db.scored(qi);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    r.n_sharing = c.n_sharing;
    r.maxCommonWords = c.max_words;
    r.minCommonWords = (int)((float)c.max_words * 0.8f);
    r.n_scored = c.n_scored;
    r.n_cand = 0;
    r.bestAccScore = loop ? q.minScore : 0.f;
    // lKFsSharingWords order: (index in the query of the first shared word, add sequence number)
    std::vector<Entry> E((size_t)c.n_scored);
    for (int i = 0; i < c.n_scored; i++)
        E[i] = Entry{h->db.slot_id(S[i].slot), S[i].words, S[i].first, h->db.slot_seq(S[i].slot), S[i].score};
    std::sort(E.begin(), E.end(),
              [](const Entry& a, const Entry& b) { return a.first != b.first ? a.first < b.first : a.seq < b.seq; });
    std::unordered_map<int32_t, float> scoreOf;   // mnLoopQuery == id && mnLoopWords > minCommonWords -> mLoopScore
    scoreOf.reserve(E.size() * 2);
    for (const Entry& e : E) scoreOf[e.id] = e.score;

    std::vector<float> acc(E.size(), nan);
    std::vector<int32_t> best(E.size(), -1);
    float bestAccScore = r.bestAccScore;
    for (size_t i = 0; i < E.size(); i++) {
        const float si = E[i].score;
        if (loop && !(si >= q.minScore)) continue;   // lScoreAndMatch (135-136)
        float bestScore = si, accScore = si;
        int32_t pBestKF = E[i].id;
        auto cv = h->covis.find(E[i].id);
        if (cv != h->covis.end())
            for (int32_t n : cv->second) {
                auto it = scoreOf.find(n);
                if (it == scoreOf.end()) continue;
                accScore += it->second;
                if (it->second > bestScore) {
                    pBestKF = n;
                    bestScore = it->second;
                }
            }
        acc[i] = accScore;
        best[i] = pBestKF;
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    r.bestAccScore = bestAccScore;
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::unordered_set<int32_t> spAlreadyAddedKF;
    int rc = ORB_OK;
    for (size_t i = 0; i < E.size(); i++) {
        if (best[i] < 0 || !(acc[i] > minScoreToRetain)) continue;
        if (!spAlreadyAddedKF.insert(best[i]).second) continue;
        if (r.n_cand < r.cap) r.cand[r.n_cand] = best[i];
        r.n_cand++;
    }
    if (r.n_cand > r.cap) rc = ORB_E_CAPACITY;
    const int m = std::min(c.n_scored, r.cap_scored);
    for (int i = 0; i < m; i++) {
        if (r.scored_id) r.scored_id[i] = E[i].id;
        if (r.scored_words) r.scored_words[i] = E[i].words;
        if (r.scored_score) r.scored_score[i] = E[i].score;
        if (r.scored_acc) r.scored_acc[i] = acc[i];
    }
    if (c.n_scored > r.cap_scored && (r.scored_id || r.scored_words || r.scored_score || r.scored_acc))
        rc = ORB_E_CAPACITY;
    return rc;
}

int detect(KeyFrameDatabase_t* h, int count, const orb_kfdb_query* q, orb_kfdb_result* r, bool loop) {
    if (count < 0 || (count > 0 && (!q || !r))) return ORB_E_INVALID;
    for (int i = 0; i < count; i++)
        if (int e = check_query(q + i, r + i, loop)) return e;
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const auto t0 = std::chrono::steady_clock::now();
    h->timed = false;
    int scoring = 0;
    const int nwords = vocab_words(h->voc, &scoring);
    if (nwords < 0 || scoring != 0) return ORB_E_INVALID;   // L1Scoring only, as ORBvocabulary_score
    for (int i = 0; i < count; i++)
        if (q[i].nq > 0 && q[i].word[q[i].nq - 1] >= (uint32_t)nwords) return ORB_E_INVALID;
    if (count == 0) return ORB_OK;
    std::vector<KfdbQuery> Q((size_t)count);
    for (int i = 0; i < count; i++)
        Q[i] = KfdbQuery{q[i].nq, q[i].word, q[i].value, loop ? q[i].n_exclude : 0, loop ? q[i].exclude : nullptr};
    h->db.enable_timing(h->timing);
    if (int e = h->db.query(count, Q.data())) return rc_of(e);
    int rc = ORB_OK;
    for (int i = 0; i < count; i++)
        if (int e = finish_query(h, i, q[i], r[i], loop)) rc = e;
    if (h->timing && h->db.timed()) {
        h->ms[0] = h->db.ms_share();
        h->ms[1] = h->db.ms_score();
        h->ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        h->timed = true;
    }
    return rc;
}

}  // namespace

extern "C" {

int KeyFrameDatabase_create(ORBvocabulary_h voc, KeyFrameDatabase_h* out) {
    if (!voc || !out) return ORB_E_INVALID;
    *out = nullptr;
    if (no_device()) return ORB_E_NODEVICE;
    auto* h = new (std::nothrow) KeyFrameDatabase_t;
    if (!h) return ORB_E_INVALID;
    h->voc = voc;
    if (int e = h->db.init(g_init_slots.load(), g_init_entries.load())) {
        delete h;
        return rc_of(e);
    }
    *out = h;
    return ORB_OK;
}

int KeyFrameDatabase_destroy(KeyFrameDatabase_h h) {
    if (!h) return ORB_E_INVALID;
    delete h;
    return ORB_OK;
}

int KeyFrameDatabase_add_batch(KeyFrameDatabase_h h, int count, const int32_t* id, const int32_t* start,
                               const uint32_t* word, const double* value) {
    if (int e = check_csr(count, id, start, word, value)) return e;
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const int nwords = vocab_words(h->voc, nullptr);
    if (nwords < 0) return ORB_E_INVALID;
    std::unordered_set<int32_t> seen;
    for (int i = 0; i < count; i++) {
        if (h->db.has(id[i]) || !seen.insert(id[i]).second) return ORB_E_INVALID;   // already listed
        const int n = start[i + 1] - start[i];
        if (n > 0 && word[start[i] + n - 1] >= (uint32_t)nwords) return ORB_E_INVALID;
    }
    return rc_of(h->db.add(count, id, start, word, value));
}

int KeyFrameDatabase_add(KeyFrameDatabase_h h, int32_t id, const uint32_t* word, const double* value, int n) {
    if (n < 0 || n > orbgpu::kKfdbMaxWords) return ORB_E_INVALID;
    const int32_t start[2] = {0, n};
    return KeyFrameDatabase_add_batch(h, 1, &id, start, word, value);
}

int KeyFrameDatabase_erase(KeyFrameDatabase_h h, int32_t id) {
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->db.erase(id));
}

int KeyFrameDatabase_clear(KeyFrameDatabase_h h) {
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    return rc_of(h->db.clear());
}

int KeyFrameDatabase_size(KeyFrameDatabase_h h, int* n_keyframes, long long* n_entries) {
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n_keyframes) *n_keyframes = h->db.n_keyframes();
    if (n_entries) *n_entries = h->db.n_entries();
    return ORB_OK;
}

int KeyFrameDatabase_set_covisibles(KeyFrameDatabase_h h, int32_t id, int n, const int32_t* ids) {
    if (id < 0 || n < 0 || n > 10 || (n > 0 && !ids)) return ORB_E_INVALID;
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (n == 0) h->covis.erase(id);
    else h->covis[id].assign(ids, ids + n);
    return ORB_OK;
}

int KeyFrameDatabase_DetectLoopCandidates(KeyFrameDatabase_h h, const orb_kfdb_query* q, orb_kfdb_result* r) {
    if (!q || !r) return ORB_E_INVALID;
    return detect(h, 1, q, r, true);
}

int KeyFrameDatabase_DetectRelocalizationCandidates(KeyFrameDatabase_h h, const orb_kfdb_query* q,
                                                    orb_kfdb_result* r) {
    if (!q || !r) return ORB_E_INVALID;
    return detect(h, 1, q, r, false);
}

int KeyFrameDatabase_DetectRelocalizationCandidates_batch(KeyFrameDatabase_h h, int count, const orb_kfdb_query* q,
                                                          orb_kfdb_result* r) {
    return detect(h, count, q, r, false);
}

int KeyFrameDatabase_enable_timing(KeyFrameDatabase_h h, int on) {
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->timing = on != 0;
    h->timed = false;
    return ORB_OK;
}

int KeyFrameDatabase_last_timings(KeyFrameDatabase_h h, float* ms3) {
    if (!ms3) return ORB_E_INVALID;
    if (!h) return no_device() ? ORB_E_NODEVICE : ORB_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->timed) return ORB_E_INVALID;
    for (int i = 0; i < 3; i++) ms3[i] = h->ms[i];
    return ORB_OK;
}

int orbgpu_unit_set_kfdb_initial_capacity(int slots, int entries) {
    if (slots < 0 || entries < 0) return 1;
    g_init_slots.store(slots > 0 ? slots : kDefaultSlots);
    g_init_entries.store(entries > 0 ? entries : kDefaultEntries);
    return 0;
}

}  // extern "C"
