// Host side of relocalisation (include/tc2li_hip.h "Relocalisation"): the keyframe database handle -- KeyFrameDatabase's add / erase /
// clear / clearMap (SF/src/KeyFrameDatabase.cc:40-107) as rows of one pool of BowVectors, host logic that needs no GPU --, its device
// copy (brought up to date by the first query after a change), the calls of tc2li_vocabulary_score_batch and
// tc2li_detect_relocalization_candidates_batch (reloc_kernels.hip), and tc2li_search_by_projection_keyframe_batch (the matcher's kernels).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "matcher_device.hpp"
#include "orb_handle.hpp"
#include "pose_opt_device.hpp"
#include "projection_search.hpp"
#include "reloc_device.hpp"
#include "tracking_device.hpp"

using namespace tc2li;

namespace {

struct DbRow {
    int32_t kf_id, map_id, seq;
    int32_t off, n;
    bool live;
    float score;                 // mRelocScore
    int32_t n_cov;
    int32_t cov[kRelocMaxNeighbours];  // kf_ids
};

}  // namespace

struct tc2li_keyframe_db {
    const tc2li_vocabulary* voc = nullptr;
    int n_voc_words = 0, scoring = 0;
    mutable std::mutex mu;
    std::vector<DbRow> rows;             // in sequence order, dead rows included until the pool is compacted
    std::vector<int32_t> word;           // the pool
    std::vector<double> value;
    std::unordered_map<int32_t, int> row_of;  // live kf_id -> row
    int next_seq = 0, dead = 0;
    // device copy
    bool rows_dirty = true;              // row table (live flags, neighbours, scores) differs from the device's
    size_t words_on_device = 0;          // pool entries the device holds; 0 after a compaction
    DevBuf<int32_t> d_word;
    DevBuf<double> d_value;
    DevBuf<RelocRowDev> d_rows;
    DevBuf<float> d_score;
    std::vector<float> score_down;       // download target of a query
};

namespace {

int voc_info(const tc2li_vocabulary* v, int* n_words, int* scoring) {
    int32_t info[6];
    if (tc2li_vocabulary_info(v, info) < 0) return TC2LI_ERR_INVALID;
    *scoring = info[2]; *n_words = info[5];
    return TC2LI_OK;
}

// a BowVector as std::map holds it: ids strictly ascending, inside the vocabulary
bool bow_ok(int n, const int32_t* w, const double* v, int n_voc_words) {
    if (n < 0 || (n > 0 && (!w || !v))) return false;
    for (int i = 0; i < n; ++i)
        if (w[i] < 0 || w[i] >= n_voc_words || (i > 0 && w[i] <= w[i - 1])) return false;
    return true;
}

void kill_row(tc2li_keyframe_db* db, int r) {
    db->rows[r].live = false;
    db->row_of.erase(db->rows[r].kf_id);
    ++db->dead;
    db->rows_dirty = true;
}

// the dead rows leave the pool when they pass half of it; sequence order is kept
void compact_if_due(tc2li_keyframe_db* db) {
    if ((size_t)db->dead * 2 <= db->rows.size()) return;
    std::vector<DbRow> rows;
    std::vector<int32_t> word;
    std::vector<double> value;
    rows.reserve(db->rows.size() - db->dead);
    for (const DbRow& r : db->rows) {
        if (!r.live) continue;
        DbRow c = r;
        c.off = (int32_t)word.size();
        word.insert(word.end(), db->word.begin() + r.off, db->word.begin() + r.off + r.n);
        value.insert(value.end(), db->value.begin() + r.off, db->value.begin() + r.off + r.n);
        db->row_of[c.kf_id] = (int)rows.size();
        rows.push_back(c);
    }
    db->rows.swap(rows); db->word.swap(word); db->value.swap(value);
    db->dead = 0;
    db->words_on_device = 0;
    db->rows_dirty = true;
}

// brings the device copy up to date (the caller holds db->mu): new pool entries are appended, the row table is rebuilt
int sync_device(tc2li_keyframe_db* db, std::vector<RelocRowDev>& stage, std::vector<float>& stage_score, hipStream_t st) {
    const size_t nw = db->word.size(), nr = db->rows.size();
    if (nw > db->d_word.n) {  // growing loses the content
        TC2LI_HIP_CHECK(hipStreamSynchronize(st));
        TC2LI_HIP_CHECK(db->d_word.ensure(nw)); TC2LI_HIP_CHECK(db->d_value.ensure(nw));
        db->words_on_device = 0;
    }
    if (nw > db->words_on_device) {
        const size_t a = db->words_on_device;
        TC2LI_HIP_CHECK(hipMemcpyAsync(db->d_word.p + a, db->word.data() + a, (nw - a) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        TC2LI_HIP_CHECK(hipMemcpyAsync(db->d_value.p + a, db->value.data() + a, (nw - a) * sizeof(double), hipMemcpyHostToDevice, st));
        db->words_on_device = nw;
    }
    if (db->rows_dirty && nr > 0) {
        if (nr > db->d_rows.n) {
            TC2LI_HIP_CHECK(hipStreamSynchronize(st));
            TC2LI_HIP_CHECK(db->d_rows.ensure(nr)); TC2LI_HIP_CHECK(db->d_score.ensure(nr));
        }
        stage.resize(nr); stage_score.resize(nr);
        for (size_t r = 0; r < nr; ++r) {
            const DbRow& s = db->rows[r];
            RelocRowDev& d = stage[r];
            d.off = s.off; d.n = s.n; d.live = s.live ? 1 : 0; d.map_id = s.map_id; d.kf_id = s.kf_id;
            d.n_cov = s.live ? s.n_cov : 0;
            for (int k = 0; k < kRelocMaxNeighbours; ++k) {
                d.cov[k] = -1;
                if (k < d.n_cov) { auto it = db->row_of.find(s.cov[k]); if (it != db->row_of.end()) d.cov[k] = it->second; }
            }
            stage_score[r] = s.score;
        }
        TC2LI_HIP_CHECK(hipMemcpyAsync(db->d_rows.p, stage.data(), nr * sizeof(RelocRowDev), hipMemcpyHostToDevice, st));
        TC2LI_HIP_CHECK(hipMemcpyAsync(db->d_score.p, stage_score.data(), nr * sizeof(float), hipMemcpyHostToDevice, st));
    }
    db->rows_dirty = false;
    return TC2LI_OK;
}

// the buffers of tc2li_vocabulary_score_batch and tc2li_detect_relocalization_candidates_batch, per host thread
PackedBuffers& rws() { static thread_local PackedBuffers w; return w; }

const char* kKlText = "scoring type KL is not supported on the device (it calls log(), whose device result is not the host library's to the last bit)";

}  // namespace

extern "C" int tc2li_keyframe_db_create(const tc2li_vocabulary* voc, tc2li_keyframe_db** out) {
    if (!voc || !out) { set_error("tc2li_keyframe_db_create: invalid argument"); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    int nw = 0, sc = 0;
    if (int rc = voc_info(voc, &nw, &sc)) return rc;
    tc2li_keyframe_db* db = new tc2li_keyframe_db();
    db->voc = voc; db->n_voc_words = nw; db->scoring = sc;
    *out = db;
    return TC2LI_OK;
}

extern "C" void tc2li_keyframe_db_destroy(tc2li_keyframe_db* db) { delete db; }

extern "C" int tc2li_keyframe_db_add(tc2li_keyframe_db* db, int32_t kf_id, int32_t map_id, int n_words, const int32_t* bow_word,
                                     const double* bow_value) {
    if (!db || kf_id < 0) { set_error("tc2li_keyframe_db_add: invalid argument"); return TC2LI_ERR_INVALID; }
    if (!bow_ok(n_words, bow_word, bow_value, db->n_voc_words)) {
        set_error("tc2li_keyframe_db_add: keyframe %d: word ids must be strictly ascending and inside the vocabulary (%d words)", kf_id, db->n_voc_words);
        return TC2LI_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->row_of.count(kf_id)) { set_error("tc2li_keyframe_db_add: keyframe %d is in the database already", kf_id); return TC2LI_ERR_INVALID; }
    if (n_words > kRelocMaxWords) { set_error("tc2li_keyframe_db_add: keyframe %d has %d words (at most %d)", kf_id, n_words, kRelocMaxWords); return TC2LI_ERR_CAPACITY; }
    if ((int)db->row_of.size() >= kRelocMaxLive) { set_error("tc2li_keyframe_db_add: the database holds %d keyframes already", kRelocMaxLive); return TC2LI_ERR_CAPACITY; }
    DbRow r{};
    r.kf_id = kf_id; r.map_id = map_id; r.seq = db->next_seq++; r.off = (int32_t)db->word.size(); r.n = n_words; r.live = true; r.score = 0.0f;
    db->word.insert(db->word.end(), bow_word, bow_word + n_words);
    db->value.insert(db->value.end(), bow_value, bow_value + n_words);
    db->row_of[kf_id] = (int)db->rows.size();
    db->rows.push_back(r);
    db->rows_dirty = true;
    return r.seq;
}

extern "C" int tc2li_keyframe_db_erase(tc2li_keyframe_db* db, int32_t kf_id) {
    if (!db) { set_error("tc2li_keyframe_db_erase: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    auto it = db->row_of.find(kf_id);
    if (it == db->row_of.end()) return 0;
    kill_row(db, it->second);
    compact_if_due(db);
    return 1;
}

extern "C" int tc2li_keyframe_db_clear(tc2li_keyframe_db* db) {
    if (!db) { set_error("tc2li_keyframe_db_clear: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    const int n = (int)db->row_of.size();
    db->rows.clear(); db->word.clear(); db->value.clear(); db->row_of.clear();
    db->dead = 0; db->words_on_device = 0; db->rows_dirty = true;
    return n;
}

extern "C" int tc2li_keyframe_db_clear_map(tc2li_keyframe_db* db, int32_t map_id) {
    if (!db) { set_error("tc2li_keyframe_db_clear_map: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    int n = 0;
    for (size_t r = 0; r < db->rows.size(); ++r)
        if (db->rows[r].live && db->rows[r].map_id == map_id) { kill_row(db, (int)r); ++n; }
    compact_if_due(db);
    return n;
}

extern "C" int tc2li_keyframe_db_size(const tc2li_keyframe_db* db) {
    if (!db) { set_error("tc2li_keyframe_db_size: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    return (int)db->row_of.size();
}

extern "C" int tc2li_keyframe_db_set_covisibility(tc2li_keyframe_db* db, int32_t kf_id, int n, const int32_t* ids) {
    if (!db || n < 0 || (n > 0 && !ids)) { set_error("tc2li_keyframe_db_set_covisibility: invalid argument"); return TC2LI_ERR_INVALID; }
    if (n > kRelocMaxNeighbours) { set_error("tc2li_keyframe_db_set_covisibility: %d neighbours (at most %d)", n, kRelocMaxNeighbours); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    auto it = db->row_of.find(kf_id);
    if (it == db->row_of.end()) { set_error("tc2li_keyframe_db_set_covisibility: keyframe %d is not in the database", kf_id); return TC2LI_ERR_INVALID; }
    DbRow& r = db->rows[it->second];
    r.n_cov = n;
    for (int k = 0; k < n; ++k) r.cov[k] = ids[k];
    db->rows_dirty = true;
    return n;
}

extern "C" int tc2li_keyframe_db_entries(const tc2li_keyframe_db* db, int capacity, int32_t* kf_id, int32_t* map_id, int32_t* sequence, float* score) {
    if (!db || capacity < 0) { set_error("tc2li_keyframe_db_entries: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(db->mu);
    const int n = (int)db->row_of.size();
    if (n > capacity) { set_error("tc2li_keyframe_db_entries: capacity %d < %d entries", capacity, n); return TC2LI_ERR_CAPACITY; }
    int i = 0;
    for (const DbRow& r : db->rows) {
        if (!r.live) continue;
        if (kf_id) kf_id[i] = r.kf_id;
        if (map_id) map_id[i] = r.map_id;
        if (sequence) sequence[i] = r.seq;
        if (score) score[i] = r.score;
        ++i;
    }
    return n;
}

extern "C" int tc2li_vocabulary_score_batch(tc2li_vocabulary* voc, int n_pairs, const tc2li_bow_vector* v1, const tc2li_bow_vector* v2,
                                            double* scores, void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    if (!voc || n_pairs < 0 || (n_pairs > 0 && (!v1 || !v2 || !scores))) { set_error("tc2li_vocabulary_score_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    int nw = 0, sc = 0;
    if (int rc = voc_info(voc, &nw, &sc)) return rc;
    if (sc == 3) { set_error("tc2li_vocabulary_score_batch: %s", kKlText); return TC2LI_ERR_INVALID; }
    std::vector<RelocPairDev> P(n_pairs);
    size_t total = 0;
    for (int p = 0; p < n_pairs; ++p) {
        for (const tc2li_bow_vector* v : {&v1[p], &v2[p]}) {
            if (!bow_ok(v->n, v->word, v->value, nw)) {
                set_error("tc2li_vocabulary_score_batch: pair %d: word ids must be strictly ascending and inside the vocabulary (%d words)", p, nw);
                return TC2LI_ERR_INVALID;
            }
            if (v->n > kRelocMaxWords) { set_error("tc2li_vocabulary_score_batch: pair %d: %d words (at most %d)", p, v->n, kRelocMaxWords); return TC2LI_ERR_CAPACITY; }
        }
        P[p] = RelocPairDev{(int32_t)total, v1[p].n, (int32_t)(total + v1[p].n), v2[p].n};
        total += (size_t)v1[p].n + v2[p].n;
    }
    if (n_pairs == 0) return 0;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    PackedTransfer T;
    const size_t t1 = std::max<size_t>(total, 1);
    const auto t_pairs = T.io.take<RelocPairDev>(n_pairs);
    const auto t_word = T.io.take<int32_t>(t1);
    const auto t_value = T.io.take<double>(t1), t_out = T.work.take<double>(n_pairs);
    T.outputs_begin();
    TC2LI_HIP_CHECK(T.ensure(rws()));
    T.io.put(t_pairs, 0, P.data(), n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        T.io.put(t_word, P[p].off1, v1[p].word, v1[p].n); T.io.put(t_value, P[p].off1, v1[p].value, v1[p].n);
        T.io.put(t_word, P[p].off2, v2[p].word, v2[p].n); T.io.put(t_value, P[p].off2, v2[p].value, v2[p].n);
    }
    TC2LI_HIP_CHECK(T.upload(st));
    launch_bow_score(T.dev(t_pairs), n_pairs, T.dev(t_word), T.dev(t_value), sc, T.dev_work(t_out), st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(scores, T.dev_work(t_out), n_pairs * sizeof(double), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return n_pairs;
}

extern "C" int tc2li_detect_relocalization_candidates_batch(const tc2li_reloc_query* queries, int n_queries, int capacity, int32_t* n_candidates,
                                                            int32_t* candidates, const tc2li_reloc_scored* scored, void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    const char* fn = "tc2li_detect_relocalization_candidates_batch";
    if (n_queries < 0 || capacity < 0 || (n_queries > 0 && (!queries || !n_candidates || (capacity > 0 && !candidates))) ||
        (scored && (scored->capacity < 0 || !scored->n_scored ||
                    (scored->capacity > 0 && (!scored->kf_id || !scored->words || !scored->si || !scored->acc_score || !scored->best_kf_id))))) {
        set_error("%s: invalid argument", fn);
        return TC2LI_ERR_INVALID;
    }
    if (n_queries > 512) { set_error("%s: %d queries (at most 512 per call)", fn, n_queries); return TC2LI_ERR_CAPACITY; }
    if (n_queries == 0) return 0;
    std::vector<tc2li_keyframe_db*> dbs(n_queries);
    int scoring = -1;
    size_t n_f = 0;
    for (int q = 0; q < n_queries; ++q) {
        const tc2li_reloc_query& Q = queries[q];
        if (!Q.db) { set_error("%s: query %d has no database", fn, q); return TC2LI_ERR_INVALID; }
        if (Q.db->scoring == 3) { set_error("%s: query %d: %s", fn, q, kKlText); return TC2LI_ERR_INVALID; }
        if (scoring >= 0 && Q.db->scoring != scoring) { set_error("%s: the databases of one call must share the scoring type", fn); return TC2LI_ERR_INVALID; }
        scoring = Q.db->scoring;
        if (!bow_ok(Q.n_words, Q.bow_word, Q.bow_value, Q.db->n_voc_words)) {
            set_error("%s: query %d: word ids must be strictly ascending and inside the vocabulary (%d words)", fn, q, Q.db->n_voc_words);
            return TC2LI_ERR_INVALID;
        }
        if (Q.n_words > kRelocMaxWords) { set_error("%s: query %d: %d words (at most %d)", fn, q, Q.n_words, kRelocMaxWords); return TC2LI_ERR_CAPACITY; }
        dbs[q] = Q.db;
        n_f += Q.n_words;
    }
    // every database once: its queries depend on each other through the score state.  Locked in address order.
    std::vector<tc2li_keyframe_db*> order(dbs);
    std::sort(order.begin(), order.end());
    if (std::adjacent_find(order.begin(), order.end()) != order.end()) {
        set_error("%s: the same database twice in one call (the queries of one database are sequential: they share its score state)", fn);
        return TC2LI_ERR_INVALID;
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(n_queries);
    for (tc2li_keyframe_db* d : order) locks.emplace_back(d->mu);

    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    size_t n_rows = 0;
    int max_rows = 0;
    for (int q = 0; q < n_queries; ++q) {
        const int n = (int)queries[q].db->rows.size();
        if (n > 2 * kRelocMaxLive) { set_error("%s: query %d: the pool holds %d rows", fn, q, n); return TC2LI_ERR_CAPACITY; }
        n_rows += n;
        max_rows = std::max(max_rows, n);
    }
    const size_t nq = n_queries, nr = std::max<size_t>(n_rows, 1), cap = std::max(capacity, 1), f1 = std::max<size_t>(n_f, 1);
    const size_t lc = std::min<size_t>(kRelocMaxLive, std::max(max_rows, 1));
    // the upload block: the frames' BowVectors and the query records; device-only: per pool row, per query, the candidate and scored lists
    PackedTransfer T;
    const auto t_word = T.io.take<int32_t>(f1);
    const auto t_value = T.io.take<double>(f1);
    const auto t_queries = T.io.take<RelocQueryDev>(nq);
    T.outputs_begin();
    const auto t_common = T.work.take<int32_t>(nr), t_first_word = T.work.take<int32_t>(nr), t_ncand = T.work.take<int32_t>(nq),
               t_nscored = T.work.take<int32_t>(nq), t_cand = T.work.take<int32_t>(nq * cap), t_sc_row = T.work.take<int32_t>(nq * lc),
               t_sc_kf_words = T.work.take<int32_t>(2 * nq * lc),  // sc_kf, sc_words: one download
               t_sc_best_row = T.work.take<int32_t>(nq * lc), t_sc_best = T.work.take<int32_t>(nq * lc);
    const auto t_si = T.work.take<float>(nr), t_sc_si_acc = T.work.take<float>(2 * nq * lc);  // sc_si, sc_acc: one download
    TC2LI_HIP_CHECK(T.ensure(rws()));
    std::vector<std::vector<RelocRowDev>> stage(n_queries);
    std::vector<std::vector<float>> stage_score(n_queries);
    size_t pos = 0, row_off = 0;
    for (int q = 0; q < n_queries; ++q) {
        const tc2li_reloc_query& Q = queries[q];
        tc2li_keyframe_db* db = Q.db;
        if (int rc = sync_device(db, stage[q], stage_score[q], st)) return rc;
        T.io.put(t_word, pos, Q.bow_word, Q.n_words); T.io.put(t_value, pos, Q.bow_value, Q.n_words);
        RelocQueryDev& D = T.host(t_queries)[q];
        D.kf_word = db->d_word.p; D.kf_value = db->d_value.p; D.rows = db->d_rows.p; D.score = db->d_score.p;
        D.n_rows = (int32_t)db->rows.size();
        D.f_off = (int32_t)pos; D.f_n = Q.n_words; D.map_id = Q.map_id; D.row_off = (int32_t)row_off; D.pad_ = 0;
        pos += Q.n_words;
        row_off += D.n_rows;
    }
    TC2LI_HIP_CHECK(T.upload(st));
    auto W = [&](auto t) { return T.dev_work(t); };
    RelocArgs A{};
    A.queries = T.dev(t_queries); A.n_queries = n_queries; A.max_rows = max_rows; A.scoring = scoring;
    A.f_word = T.dev(t_word); A.f_value = T.dev(t_value);
    A.common = W(t_common); A.first_word = W(t_first_word); A.n_candidates = W(t_ncand); A.n_scored = W(t_nscored); A.candidates = W(t_cand);
    A.sc_row = W(t_sc_row); A.sc_kf = W(t_sc_kf_words); A.sc_words = A.sc_kf + nq * lc; A.sc_best_row = W(t_sc_best_row); A.sc_best = W(t_sc_best);
    A.si = W(t_si); A.sc_si = W(t_sc_si_acc); A.sc_acc = A.sc_si + nq * lc;
    A.capacity = capacity; A.list_cap = (int)lc;
    TC2LI_HIP_CHECK(hipMemsetAsync(A.candidates, 0xff, nq * cap * sizeof(int32_t), st));
    launch_reloc_candidates(A, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    // results; the score states come back to the handles, which own them
    std::vector<int32_t> n_scored(nq);
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_candidates, A.n_candidates, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_scored.data(), A.n_scored, nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (capacity > 0) TC2LI_HIP_CHECK(hipMemcpyAsync(candidates, A.candidates, nq * cap * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    for (int q = 0; q < n_queries; ++q) {
        tc2li_keyframe_db* db = dbs[q];
        db->score_down.resize(db->rows.size());
        if (!db->rows.empty())
            TC2LI_HIP_CHECK(hipMemcpyAsync(db->score_down.data(), db->d_score.p, db->rows.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    for (int q = 0; q < n_queries; ++q) {
        tc2li_keyframe_db* db = dbs[q];
        for (size_t r = 0; r < db->rows.size(); ++r) db->rows[r].score = db->score_down[r];
    }
    int rc = n_queries;
    for (int q = 0; q < n_queries && rc >= 0; ++q) {
        if (n_candidates[q] > capacity) { set_error("%s: query %d has %d candidates, capacity %d", fn, q, n_candidates[q], capacity); rc = TC2LI_ERR_CAPACITY; }
        else if (scored && n_scored[q] > scored->capacity) {
            set_error("%s: query %d scored %d keyframes, the scored list's capacity is %d", fn, q, n_scored[q], scored->capacity);
            rc = TC2LI_ERR_CAPACITY;
        }
    }
    if (rc < 0) return rc;
    if (scored) {
        memcpy(scored->n_scored, n_scored.data(), nq * sizeof(int32_t));
        const size_t sc = scored->capacity;
        if (sc > 0) {
            std::vector<int32_t> h_i(3 * nq * lc);
            std::vector<float> h_f(2 * nq * lc);
            TC2LI_HIP_CHECK(hipMemcpyAsync(h_i.data(), A.sc_kf, 2 * nq * lc * sizeof(int32_t), hipMemcpyDeviceToHost, st));  // sc_kf, sc_words
            TC2LI_HIP_CHECK(hipMemcpyAsync(h_i.data() + 2 * nq * lc, A.sc_best, nq * lc * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            TC2LI_HIP_CHECK(hipMemcpyAsync(h_f.data(), A.sc_si, 2 * nq * lc * sizeof(float), hipMemcpyDeviceToHost, st));    // sc_si, sc_acc
            TC2LI_HIP_CHECK(stream_wait_blocking(st));
            for (size_t q = 0; q < nq; ++q) {
                const size_t n = n_scored[q];
                for (size_t i = 0; i < sc; ++i) {
                    const bool in = i < n;
                    scored->kf_id[q * sc + i] = in ? h_i[q * lc + i] : -1;
                    scored->words[q * sc + i] = in ? h_i[nq * lc + q * lc + i] : 0;
                    scored->best_kf_id[q * sc + i] = in ? h_i[2 * nq * lc + q * lc + i] : -1;
                    scored->si[q * sc + i] = in ? h_f[q * lc + i] : 0.0f;
                    scored->acc_score[q * sc + i] = in ? h_f[nq * lc + q * lc + i] : 0.0f;
                }
            }
        }
    }
    return n_queries;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (SF/src/ORBmatcher.cc:1898-2019) for a batch of items.  The
// queries come from k_track_queries_keyframe; the search is the matcher's (matcher_kernels.hip: feature grid, candidate lists, the rounds
// that reproduce "a matched keypoint blocks later points") with ORBdist as its distance bound; the rotation filter is k_track_count.
namespace {

struct KfSearchWs {
    PackedBuffers b;
    SearchScratch s;
};
KfSearchWs& kws() { static thread_local KfSearchWs w; return w; }

}  // namespace

extern "C" int tc2li_search_by_projection_keyframe_batch(const tc2li_projection_keyframe_item* items, int n_items, const float* cam4,
                                                         const float* scale_factors, int n_levels, float log_scale_factor, float th, int orb_dist,
                                                         int check_orientation, int capacity, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches,
                                                         void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    const char* fn = "tc2li_search_by_projection_keyframe_batch";
    if (n_items < 0 || capacity < 0 || (n_items > 0 && (!items || !kf_keypoint_of_keypoint || !n_matches)) || !cam4 || !scale_factors || n_levels < 1 ||
        n_levels > kMaxLevels) {
        set_error("%s: invalid argument (at most %d levels)", fn, kMaxLevels);
        return TC2LI_ERR_INVALID;
    }
    if (n_items == 0) return 0;
    size_t nk = 0, nq = 0;
    for (int f = 0; f < n_items; ++f) {
        const tc2li_projection_keyframe_item& I = items[f];
        if (I.n < 0 || I.n_points < 0 || (I.n > 0 && (!I.keys || !I.descriptors || !I.held)) ||
            (I.n_points > 0 && (!I.has_point || !I.found || !I.Xw || !I.point_descriptors || !I.min_distance || !I.max_distance || !I.max_distance_raw ||
                                !I.angle))) {
            set_error("%s: item %d has null arrays", fn, f);
            return TC2LI_ERR_INVALID;
        }
        if (int rc = check_capacity(fn, I.n, capacity, f)) return rc;
        if (int rc = check_match_keys(fn, I.n, f)) return rc;
        nk += I.n; nq += I.n_points;
    }
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    KfSearchWs& w = kws();
    SearchScratch& S = w.s;
    const size_t nf = n_items, k1 = std::max<size_t>(nk, 1), q1 = std::max<size_t>(nq, 1), cap1 = std::max(capacity, 1);
    const int total_q = (int)nq;
    // the upload block: per frame keypoint the matcher's key, descriptor, angle, held flag and a u_right of -1 (the overload has no stereo
    // test); per keyframe keypoint the point; per frame the records.  Device-only: the keypoints' keyframe keypoints.
    PackedTransfer T;
    const auto t_keys = T.io.take<MatchKey>(k1);
    const auto t_desc = T.io.take<OrbDescriptor>(k1);
    const auto t_ang = T.io.take<float>(k1), t_ur = T.io.take<float>(k1);
    const auto t_held = T.io.take<uint8_t>(k1), t_found = T.io.take<uint8_t>(q1);
    const KeyframePointTables pts = take_keyframe_points(T.io, q1);
    const auto t_frames = T.io.take<TrackFrameDev>(nf);
    const auto t_bounds = T.io.take<float4>(nf);
    const auto t_mframes = T.io.take<MatchFrameDev>(nf);
    const auto t_kbase = T.io.take<int32_t>(nf), t_of_key = T.work.take<int32_t>(nf * cap1);
    T.outputs_begin();
    TC2LI_HIP_CHECK(T.ensure(w.b));
    if (int rc = S.ensure(n_items, total_q, capacity)) return rc;
    MatchKey* hk = T.host(t_keys);
    float *hang = T.host(t_ang), *hur = T.host(t_ur);
    uint8_t *hheld = T.host(t_held), *hfound = T.host(t_found);
    TrackFrameDev* hf = T.host(t_frames);
    size_t key = 0, q = 0;
    for (int f = 0; f < n_items; ++f) {
        const tc2li_projection_keyframe_item& I = items[f];
        for (int i = 0; i < I.n; ++i) {
            hk[key + i] = MatchKey{I.keys[i].x, I.keys[i].y, I.keys[i].octave};
            hang[key + i] = I.keys[i].angle;
            hur[key + i] = -1.0f;
            hheld[key + i] = I.held[i] ? 1 : 0;
        }
        T.io.put(t_desc, key, I.descriptors, I.n);
        stage_keyframe_points(T, pts, q, I);
        for (int i = 0; i < I.n_points; ++i) hfound[q + i] = I.found[i] ? 1 : 0;
        TrackFrameDev& F = hf[f];
        memset(&F, 0, sizeof(F));
        memcpy(F.pose7, I.pose7, 7 * sizeof(float));
        F.th = th; F.q_off = (int32_t)q; F.n_q = I.n_points; F.key_off = (int32_t)key; F.n_keys = I.n; F.slot = f;
        T.io.put(t_bounds, f, I.bounds, 1);
        T.host(t_mframes)[f] = MatchFrameDev{T.dev(t_keys) + key, T.dev(t_desc)[key].b, T.dev(t_ur) + key, T.dev(t_held) + key, S.d_queries.p + q,
                                             I.n, I.n_points, (int32_t)q, 0, I.bounds[0], I.bounds[1], I.bounds[2], I.bounds[3]};
        T.host(t_kbase)[f] = (int32_t)key;
        key += I.n; q += I.n_points;
    }
    const TrackConst C = track_const(cam4, scale_factors, n_levels, log_scale_factor, capacity);
    TC2LI_HIP_CHECK(T.upload(st));
    const TrackFrameDev* d_frames = T.dev(t_frames);
    const KeyframePointArrays A = keyframe_point_arrays(T, pts, T.dev(t_found));
    int32_t* d_of_key = T.dev_work(t_of_key);
    TC2LI_HIP_CHECK(hipMemsetAsync(d_of_key, 0xff, nf * cap1 * sizeof(int32_t), st));
    TC2LI_HIP_CHECK(hipMemsetAsync(S.d_nmatch.p, 0, nf * sizeof(int32_t), st));
    if (total_q > 0) {
        TC2LI_HIP_CHECK(hipMemsetAsync(S.amb_count(), 0, sizeof(int32_t), st));
        launch_track_queries_keyframe(d_frames, n_items, T.dev(t_bounds), C, A, total_q, S.d_queries.p, S.d_query_frame.p,
                                      S.d_match.p, S.amb_count(), S.d_amb_ids.p, S.d_amb_ratio.p, S.d_amb_r.p, st);
        if (int rc = resolve_ambiguous_levels(S, C, launch_track_patch_levels_keyframe, st)) return rc;
        // the follow-up kernels go behind the overflow decision: k_track_assign_keyframe scatters into of_key and must not see a partial list
        const SearchPass P{T.dev(t_mframes), T.dev(t_kbase), n_items, total_q, hf, nullptr, 0, 0.0f, orb_dist};
        if (int rc = projection_search(S, P, st)) return rc;
        launch_track_count(d_frames, nullptr, n_items, S.d_queries.p, T.dev(t_ang), check_orientation ? 1 : 0, S.d_match.p, S.d_nmatch.p, st);
        launch_track_assign_keyframe(d_frames, n_items, capacity, total_q, S.d_match.p, d_of_key, st);
        TC2LI_HIP_CHECK(hipGetLastError());
    }
    if (capacity > 0) TC2LI_HIP_CHECK(hipMemcpyAsync(kf_keypoint_of_keypoint, d_of_key, nf * cap1 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_matches, S.d_nmatch.p, nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return n_items;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The refinement ladder of Tracking::Relocalization after a PnP pose (SF/src/Tracking.cc:3562-3631) for a batch of independent hypotheses
// on the frames of the last tc2li_orb_extract_batch call: one stream, one staging upload, every branch decided on the device
// (reloc_kernels.hip k_reloc_ladder_*).  The host waits only where the searches need it: the host's logf for PredictScale on a level boundary
// and the candidate pool's overflow flag, as in tc2li_track_local_map_batch.
namespace {

struct LadderWs {
    PackedBuffers b;
    SearchScratch s;
};
LadderWs& lws() { static thread_local LadderWs w; return w; }

}  // namespace

extern "C" int tc2li_relocalization_refine_batch(tc2li_orb* o, const tc2li_reloc_hypothesis* hyps, int n_hyps, int n_frames, const float* u_right,
                                                 int capacity, const tc2li_camera* cam, int32_t* status, int32_t* n_good, int32_t* n_additional,
                                                 double* poses7, int32_t* kf_keypoint_of_keypoint, uint8_t* outlier, void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    const char* fn = "tc2li_relocalization_refine_batch";
    if (!o || n_hyps < 0 || n_frames < 0 || capacity < 0 || !u_right || !cam ||
        (n_hyps > 0 && (!hyps || !status || !n_good || !n_additional || !poses7 || !kf_keypoint_of_keypoint || !outlier))) {
        set_error("%s: invalid argument", fn);
        return TC2LI_ERR_INVALID;
    }
    if (n_hyps == 0) return 0;
    if (!orb_features_ready(o, n_frames, fn)) return TC2LI_ERR_INVALID;
    const int n_levels = o->prm.nlevels;
    if (n_levels > kMaxLevels) { set_error("%s: %d levels (at most %d)", fn, n_levels, kMaxLevels); return TC2LI_ERR_INVALID; }
    size_t nq = 0;
    for (int h = 0; h < n_hyps; ++h) {
        const tc2li_reloc_hypothesis& Hy = hyps[h];
        if (Hy.frame_index < 0 || Hy.frame_index >= n_frames) { set_error("%s: hypothesis %d names frame %d of %d", fn, h, Hy.frame_index, n_frames); return TC2LI_ERR_INVALID; }
        if (Hy.n_points < 0 || !Hy.match || !Hy.inlier ||
            (Hy.n_points > 0 && (!Hy.has_point || !Hy.Xw || !Hy.point_descriptors || !Hy.min_distance || !Hy.max_distance || !Hy.max_distance_raw || !Hy.angle))) {
            set_error("%s: hypothesis %d has null arrays", fn, h);
            return TC2LI_ERR_INVALID;
        }
        const int n = o->last_kp_cnt[2 * Hy.frame_index];
        if (int rc = check_capacity(fn, n, capacity)) return rc;
        if (int rc = check_match_keys(fn, n)) return rc;
        for (int i = 0; i < n; ++i)
            if (Hy.inlier[i] && (Hy.match[i] < -1 || Hy.match[i] >= Hy.n_points)) {
                set_error("%s: hypothesis %d: match[%d] = %d is no keypoint of the keyframe (%d)", fn, h, i, Hy.match[i], Hy.n_points);
                return TC2LI_ERR_INVALID;
            }
        nq += Hy.n_points;
    }
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    LadderWs& w = lws();
    SearchScratch& S = w.s;
    const size_t nh = n_hyps, cap1 = std::max(capacity, 1), q1 = std::max<size_t>(nq, 1), ne = nh * cap1, nfr = std::max(n_frames, 1);
    const int total_q = (int)nq;
    // the upload block: the keyframes' points, the hypotheses' matches and inlier flags, mvuRight, a row of -1 (the search has no stereo
    // test), the records per hypothesis
    PackedTransfer T;
    const KeyframePointTables pts = take_keyframe_points(T.io, q1);
    const auto t_match = T.io.take<int32_t>(ne), t_kbase = T.io.take<int32_t>(nh), t_foh = T.io.take<int32_t>(nh);
    const auto t_inl = T.io.take<uint8_t>(ne);
    const auto t_ur = T.io.take<float>(nfr * cap1), t_neg = T.io.take<float>(cap1);
    const auto t_frames = T.io.take<TrackFrameDev>(nh);
    const auto t_bounds = T.io.take<float4>(nh);
    const auto t_mframes = T.io.take<MatchFrameDev>(nh);
    T.outputs_begin();
    // device-only: the ladder's state per hypothesis, per keypoint and per keyframe point, PoseOptimization's tables
    const auto t_active = T.work.take<int32_t>(nh), t_status = T.work.take<int32_t>(nh), t_ngood = T.work.take<int32_t>(nh),
               t_nadd = T.work.take<int32_t>(2 * nh), t_assign = T.work.take<int32_t>(ne);
    const auto t_found = T.work.take<uint8_t>(q1), t_occ = T.work.take<uint8_t>(ne), t_outl_key = T.work.take<uint8_t>(ne);
    const auto t_stage_poses = T.work.take<double>(21 * nh);
    const PoseTail pose(T.work, nh, ne);
    TC2LI_HIP_CHECK(T.ensure(w.b));
    if (int rc = S.ensure(n_hyps, total_q, capacity)) return rc;
    FrameGrids G;  // the handle's grids: hypothesis k reads the row of its frame (frame_of_hyp), the items start where the frame's keys start
    if (int rc = frame_grids(o, st, &G)) return rc;
    auto W = [&](auto t) { return T.dev_work(t); };
    memset(T.host(t_match), 0xff, ne * sizeof(int32_t));
    memset(T.host(t_inl), 0, ne);
    T.io.put(t_ur, 0, u_right, (size_t)n_frames * capacity);
    for (size_t i = 0; i < cap1; ++i) T.host(t_neg)[i] = -1.0f;  // the overload has no stereo test
    TrackFrameDev* hf = T.host(t_frames);
    size_t q = 0;
    for (int k = 0; k < n_hyps; ++k) {
        const tc2li_reloc_hypothesis& Hy = hyps[k];
        const int n = o->last_kp_cnt[2 * Hy.frame_index], key_off = o->last_kp_off[2 * Hy.frame_index];
        stage_keyframe_points(T, pts, q, Hy);
        T.io.put(t_match, (size_t)k * cap1, Hy.match, n);
        for (int i = 0; i < n; ++i) T.host(t_inl)[(size_t)k * cap1 + i] = Hy.inlier[i] ? 1 : 0;
        TrackFrameDev& F = hf[k];
        memset(&F, 0, sizeof(F));
        memcpy(F.pose7, Hy.pose7, 7 * sizeof(float));
        F.th = 10.0f; F.q_off = (int32_t)q; F.n_q = Hy.n_points; F.key_off = key_off; F.n_keys = n; F.slot = -1;
        const float B[4] = {0.0f, (float)o->cur_w, 0.0f, (float)o->cur_h};
        T.io.put(t_bounds, k, B, 1);
        T.host(t_mframes)[k] = MatchFrameDev{o->d_mkeys.p + key_off, o->d_desc.p + (size_t)key_off * 32, T.dev(t_neg), W(t_occ) + (size_t)k * cap1,
                                             S.d_queries.p + q, n, Hy.n_points, (int32_t)q, 0, B[0], B[1], B[2], B[3]};
        T.host(t_kbase)[k] = G.cell_start ? key_off : (int32_t)(k * cap1);
        T.host(t_foh)[k] = Hy.frame_index;
        q += Hy.n_points;
    }
    const TrackConst C = track_const(o, cam, 0.f, capacity);
    TC2LI_HIP_CHECK(T.upload(st));
    TrackFrameDev* d_frames = T.dev(t_frames);  // the ladder rewrites pose, window and slot on the device; the host records stay as sent
    int32_t *d_nm = S.d_nmatch.p, *d_assign = W(t_assign);
    const KeyframePointArrays A = keyframe_point_arrays(T, pts, W(t_found));
    RelocLadder L{};
    L.n_hyps = n_hyps; L.capacity = (int)cap1; L.frames = d_frames; L.frame_of_hyp = T.dev(t_foh);
    L.keys = o->d_mkeys.p; L.u_right = T.dev(t_ur);
    for (int l = 0; l < n_levels; ++l) L.inv_sigma2[l] = o->inv_sigma2[l];
    L.kf_Xw = A.Xw; L.in_match = T.dev(t_match); L.in_inlier = T.dev(t_inl);
    L.found = W(t_found); L.occupied = W(t_occ); L.assign = d_assign; L.outlier_of_key = W(t_outl_key); L.n_matches = d_nm; L.active = W(t_active);
    L.status = W(t_status); L.n_good = W(t_ngood); L.n_additional = W(t_nadd); L.stage_poses = W(t_stage_poses);
    L.probs = W(pose.probs); L.edges = W(pose.edges); L.Xw = W(pose.Xw); L.edge_kp = W(pose.edge_kp); L.poses = W(pose.poses);
    L.outlier = W(pose.outlier); L.inliers = W(pose.inliers);
    // ORBmatcher matcher2(0.9, true).SearchByProjection(mCurrentFrame, pKF, sFound, th, orb_dist) for the hypotheses k_reloc_ladder_after chose
    auto search = [&](int orb_dist) -> int {
        if (total_q == 0) return TC2LI_OK;
        TC2LI_HIP_CHECK(hipMemsetAsync(S.amb_count(), 0, sizeof(int32_t), st));
        launch_track_queries_keyframe(d_frames, n_hyps, T.dev(t_bounds), C, A, total_q, S.d_queries.p, S.d_query_frame.p,
                                      S.d_match.p, S.amb_count(), S.d_amb_ids.p, S.d_amb_ratio.p, S.d_amb_r.p, st);
        if (int rc = resolve_ambiguous_levels(S, C, launch_track_patch_levels_keyframe, st)) return rc;
        const SearchPass P{T.dev(t_mframes), T.dev(t_kbase), n_hyps, total_q, hf, nullptr,
                           0, 0.0f, orb_dist, G.cell_start, G.items, G.cell_start ? L.frame_of_hyp : nullptr};
        if (int rc = projection_search(S, P, st)) return rc;  // the follow-up waits for the overflow decision: assign scatters
        launch_track_count(d_frames, nullptr, n_hyps, S.d_queries.p, o->d_angles.p, 1, S.d_match.p, d_nm, st);
        launch_track_assign_keyframe(d_frames, n_hyps, (int)cap1, total_q, S.d_match.p, d_assign, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        return TC2LI_OK;
    };
    launch_reloc_ladder_init(L, st);
    for (int stage = 0; stage < 3; ++stage) {
        launch_reloc_ladder_edges(L, stage, st);
        pose.launch(T, n_hyps, cam, (int)cap1, st);
        launch_reloc_ladder_after(L, stage, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        if (stage < 2) { if (int rc = search(stage == 0 ? 100 : 64)) return rc; }
    }
    TC2LI_HIP_CHECK(hipMemcpyAsync(status, L.status, nh * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_good, L.n_good, nh * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_additional, L.n_additional, 2 * nh * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(poses7, L.stage_poses, 21 * nh * sizeof(double), hipMemcpyDeviceToHost, st));
    if (capacity > 0) {
        TC2LI_HIP_CHECK(hipMemcpyAsync(kf_keypoint_of_keypoint, d_assign, ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(hipMemcpyAsync(outlier, L.outlier_of_key, ne, hipMemcpyDeviceToHost, st));
    }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return n_hyps;
}
