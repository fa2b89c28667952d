// Host side of the ORB vocabulary (include/tc2li_hip.h "ORB vocabulary"): the handle -- DBoW2's text format
// (TemplatedVocabulary::loadFromTextFile, SF/Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1350-1436) or the same content from arrays,
// host logic that needs no GPU --, its device copy (made on first device use, once per handle), and the calls of
// tc2li_vocabulary_transform_batch, tc2li_orb_compute_bow_batch and tc2li_search_by_bow_batch (bow_kernels.hip).
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bow_device.hpp"
#include "common.hpp"
#include "orb_handle.hpp"
#include "pose_opt_device.hpp"
#include "projection_search.hpp"

using namespace tc2li;

struct tc2li_vocabulary {
    int k = 0, L = 0, scoring = 0, weighting = 0;
    int n_words = 0;
    // reference numbering: node 0 is the root, node i > 0 is the i-th line of the file
    std::vector<int32_t> parent, word;     // word id, -1 for a node that is not a word
    std::vector<uint8_t> desc;             // [nodes][32]
    std::vector<double> weight;
    std::vector<std::vector<int32_t>> children;
    // device copy (bow_device.hpp), made on first use
    std::mutex mu;
    bool on_device = false;
    DevBuf<uint4> d_rows;
    DevBuf<BowNodeDev> d_nodes;
    DevBuf<double> d_weight, d_word_weight;

    int n_nodes() const { return (int)parent.size(); }
};

namespace {

// nodes 1 .. n in file order -> the handle; the checks of the loader (line numbers are the file's, `line_of` NULL for arrays)
int build_vocabulary(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const int32_t* is_leaf, const uint8_t* desc,
                     const double* weights, const int* line_of, tc2li_vocabulary** out) {
    auto where = [&](int i) { return line_of ? std::string("line ") + std::to_string(line_of[i]) : std::string("node ") + std::to_string(i + 1); };
    if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3) {
        set_error("vocabulary: bad header (k %d, L %d, scoring %d, weighting %d): 0 <= k <= 20, 1 <= L <= 10, 0 <= scoring <= 5, "
                  "0 <= weighting <= 3", k, L, scoring, weighting);
        return TC2LI_ERR_INVALID;
    }
    if (n < 0 || (n > 0 && (!parent || !is_leaf || !desc || !weights))) { set_error("vocabulary: invalid node arrays"); return TC2LI_ERR_INVALID; }
    tc2li_vocabulary* v = new tc2li_vocabulary();
    v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
    v->parent.assign(n + 1, -1); v->word.assign(n + 1, -1); v->desc.assign((size_t)(n + 1) * 32, 0); v->weight.assign(n + 1, 0.0);
    v->children.assign(n + 1, {});
    std::vector<uint8_t> flagged(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int id = i + 1, p = parent[i];
        if (p < 0 || p >= id) { set_error("vocabulary: %s: parent %d is not an earlier node", where(i).c_str(), p); delete v; return TC2LI_ERR_INVALID; }
        if (flagged[p]) { set_error("vocabulary: %s: parent %d is a word and cannot have children", where(i).c_str(), p); delete v; return TC2LI_ERR_INVALID; }
        if (v->children[p].size() >= 65535) {
            set_error("vocabulary: %s: node %d would have more than 65535 children", where(i).c_str(), p);
            delete v;
            return TC2LI_ERR_INVALID;
        }
        v->parent[id] = p;
        v->children[p].push_back(id);
        memcpy(&v->desc[(size_t)id * 32], desc + (size_t)i * 32, 32);
        v->weight[id] = weights[i];
        if (is_leaf[i] > 0) { flagged[id] = 1; v->word[id] = v->n_words++; }
    }
    for (int i = 0; i < n; ++i)
        if (!flagged[i + 1] && v->children[i + 1].empty()) {
            set_error("vocabulary: %s: node %d has no children and is not flagged as a word", where(i).c_str(), i + 1);
            delete v;
            return TC2LI_ERR_INVALID;
        }
    *out = v;
    return TC2LI_OK;
}

// the device copy: breadth-first renumbering, so that the children of every node are one contiguous block of rows in child order
int ensure_device(tc2li_vocabulary* v) {
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->on_device) return TC2LI_OK;
    const int n = v->n_nodes();
    std::vector<int32_t> order;  // device index -> reference id
    order.reserve(n);
    order.push_back(0);
    std::vector<BowNodeDev> nodes(n);
    for (size_t q = 0; q < order.size(); ++q) {
        const int id = order[q];
        BowNodeDev& d = nodes[q];
        d.first = v->children[id].empty() ? 0 : (int32_t)order.size();
        d.cnt = (int32_t)v->children[id].size();
        d.ref = id;
        d.word = v->word[id];
        for (int c : v->children[id]) order.push_back(c);
    }
    std::vector<uint4> rows((size_t)n * 2);
    std::vector<double> w(n), ww(std::max(v->n_words, 1), 0.0);
    for (int q = 0; q < n; ++q) {
        memcpy(&rows[2 * (size_t)q], &v->desc[(size_t)order[q] * 32], 32);
        w[q] = v->weight[order[q]];
        if (v->word[order[q]] >= 0) ww[v->word[order[q]]] = w[q];
    }
    hipStream_t st = private_stream();
    TC2LI_HIP_CHECK(v->d_rows.alloc(rows.size())); TC2LI_HIP_CHECK(v->d_nodes.alloc(n));
    TC2LI_HIP_CHECK(v->d_weight.alloc(n)); TC2LI_HIP_CHECK(v->d_word_weight.alloc(ww.size()));
    TC2LI_HIP_CHECK(hipMemcpyAsync(v->d_rows.p, rows.data(), rows.size() * sizeof(uint4), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(v->d_nodes.p, nodes.data(), n * sizeof(BowNodeDev), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(v->d_weight.p, w.data(), n * sizeof(double), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(v->d_word_weight.p, ww.data(), ww.size() * sizeof(double), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    v->on_device = true;
    return TC2LI_OK;
}

BowVocDev voc_dev(const tc2li_vocabulary* v) {
    return BowVocDev{v->d_rows.p, v->d_nodes.p, v->d_weight.p, v->n_nodes(), v->n_words};
}

// the buffers of the entries below, per host thread
PackedBuffers& bws() { static thread_local PackedBuffers w; return w; }

bool out_ok(const tc2li_bow_out* o) {
    return o && o->word && o->node && o->n_words && o->bow_word && o->bow_value && o->n_nodes && o->fv_node && o->fv_offset && o->fv_index;
}

// The tables of a transform of nf frames over `total` descriptor rows, taken from the caller's transfer: the frame records go up in its
// block, the rest is device-only.  The int32 arrays are one table, filled in one go: word, node, bow_word, fv_node, fv_index, rank,
// flags [nt] each; fv_offset [nt + nf]; n_words, n_nodes, n_valid [nf].
struct BowTransform {
    int nf;
    size_t nt;
    Table<BowFrameDev> frames;
    Table<int32_t> i32;
    Table<double> bow_value;
    BowTransform(PackedTransfer& T, int n_frames, size_t total) : nf(n_frames), nt(std::max<size_t>(total, 1)) {
        frames = T.io.take<BowFrameDev>(nf); i32 = T.work.take<int32_t>(8 * nt + 4 * (size_t)nf); bow_value = T.work.take<double>(nt);
    }
};

// after T.ensure(): the frame records into the block.  After T.upload(), descriptors on the device at `desc` (rows src_row ..): queues the
// descent and the assembly into the transform's arrays (O)
int queue_transform(tc2li_vocabulary* v, const PackedTransfer& T, const BowTransform& B, const uint8_t* desc, int levelsup, BowOutDev& O, hipStream_t st) {
    const size_t nt = B.nt, nf = B.nf;
    int32_t* p = T.dev_work(B.i32);
    O.word = p; O.node = p + nt; O.bow_word = p + 2 * nt; O.fv_node = p + 3 * nt; O.fv_index = p + 4 * nt;
    O.rank = reinterpret_cast<uint32_t*>(p + 5 * nt); O.flags = p + 6 * nt; O.fv_offset = p + 7 * nt;
    O.n_words = p + 8 * nt + nf; O.n_nodes = O.n_words + nf; O.n_valid = O.n_nodes + nf;
    O.bow_value = T.dev_work(B.bow_value);
    int max_n = 0;
    for (size_t f = 0; f < nf; ++f) max_n = std::max(max_n, T.host(B.frames)[f].n);
    // entries beyond a frame's counts read back as -1 / 0 on every call
    TC2LI_HIP_CHECK(hipMemsetAsync(p, 0xff, (8 * nt + 4 * nf) * sizeof(int32_t), st));
    TC2LI_HIP_CHECK(hipMemsetAsync(O.bow_value, 0, nt * sizeof(double), st));
    const BowVocDev V = voc_dev(v);
    launch_bow_descend(V, desc, T.dev(B.frames), B.nf, max_n, v->L - levelsup, O, st);
    launch_bow_assemble(V, v->d_word_weight.p, T.dev(B.frames), B.nf, v->scoring, v->weighting, O, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    return TC2LI_OK;
}

// the downloads of a queued transform into the caller's arrays (no wait)
int queue_transform_download(const BowOutDev& O, size_t total, int nf, const tc2li_bow_out* out, hipStream_t st) {
    auto down = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    TC2LI_HIP_CHECK(down(out->word, O.word, total * 4));
    TC2LI_HIP_CHECK(down(out->node, O.node, total * 4));
    TC2LI_HIP_CHECK(down(out->bow_word, O.bow_word, total * 4));
    TC2LI_HIP_CHECK(down(out->bow_value, O.bow_value, total * 8));
    TC2LI_HIP_CHECK(down(out->fv_node, O.fv_node, total * 4));
    TC2LI_HIP_CHECK(down(out->fv_index, O.fv_index, total * 4));
    TC2LI_HIP_CHECK(down(out->fv_offset, O.fv_offset, (total + nf) * 4));
    TC2LI_HIP_CHECK(down(out->n_words, O.n_words, nf * 4));
    TC2LI_HIP_CHECK(down(out->n_nodes, O.n_nodes, nf * 4));
    return TC2LI_OK;
}

// The transform alone.  The descriptors are on the device at dev_desc, or, dev_desc NULL, `total` rows of the caller's at host_desc, which go
// up to a table of the call.
int run_transform(tc2li_vocabulary* v, const uint8_t* dev_desc, const uint8_t* host_desc, const std::vector<BowFrameDev>& frames, size_t total, int levelsup,
                  const tc2li_bow_out* out, hipStream_t st) {
    PackedTransfer T;
    const BowTransform B(T, (int)frames.size(), total);
    T.outputs_begin();
    const Table<OrbDescriptor> t_desc = T.work.take<OrbDescriptor>(dev_desc ? 0 : B.nt);
    TC2LI_HIP_CHECK(T.ensure(bws()));
    T.io.put(B.frames, 0, frames.data(), frames.size());
    TC2LI_HIP_CHECK(T.upload(st));
    if (!dev_desc) {
        if (total) TC2LI_HIP_CHECK(hipMemcpyAsync(T.dev_work(t_desc), host_desc, total * sizeof(OrbDescriptor), hipMemcpyHostToDevice, st));
        dev_desc = T.dev_work(t_desc)->b;
    }
    BowOutDev O;
    if (int rc = queue_transform(v, T, B, dev_desc, levelsup, O, st)) return rc;
    if (int rc = queue_transform_download(O, total, B.nf, out, st)) return rc;
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return B.nf;
}

// a FeatureVector as tc2li_search_for_triangulation checks it (mapping_host.cpp): offsets from 0, not decreasing, nodes strictly ascending,
// feature indices in [0, n)
bool feature_vector_ok(const tc2li_keyframe_view& V) {
    if (V.n_nodes == 0) return true;
    if (V.fv_offset[0] != 0) return false;
    for (int a = 0; a < V.n_nodes; ++a) {
        if (V.fv_offset[a + 1] < V.fv_offset[a]) return false;
        if (a > 0 && V.fv_node[a] <= V.fv_node[a - 1]) return false;
    }
    for (int i = 0; i < V.fv_offset[V.n_nodes]; ++i)
        if (V.fv_index[i] < 0 || V.fv_index[i] >= V.n) return false;
    return true;
}

}  // namespace

extern "C" int tc2li_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent, const int32_t* is_leaf,
                                       const uint8_t* descriptors, const double* weights, tc2li_vocabulary** out) {
    if (!out) { set_error("tc2li_vocabulary_create: out is NULL"); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    return build_vocabulary(k, L, scoring, weighting, n_nodes, parent, is_leaf, descriptors, weights, nullptr, out);
}

extern "C" int tc2li_vocabulary_load_text(const char* path, tc2li_vocabulary** out) {
    if (!path || !out) { set_error("tc2li_vocabulary_load_text: invalid argument"); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    FILE* fp = fopen(path, "rb");
    if (!fp) { set_error("vocabulary: cannot read %s: %s", path, strerror(errno)); return TC2LI_ERR_INVALID; }
    std::string text;
    {
        char buf[1 << 16];
        size_t r;
        while ((r = fread(buf, 1, sizeof(buf), fp)) > 0) text.append(buf, r);
        const bool bad = ferror(fp) != 0;
        fclose(fp);
        if (bad) { set_error("vocabulary: cannot read %s", path); return TC2LI_ERR_INVALID; }
    }
    // whitespace as operator>> sees it, '\r' included; blank lines are skipped (see the header)
    auto is_space = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; };
    const char* s = text.c_str();
    const char* end = s + text.size();
    int line_no = 0;
    bool have_header = false;
    int hdr[4] = {0, 0, 0, 0};
    std::vector<int32_t> parent, is_leaf;
    std::vector<uint8_t> desc;
    std::vector<double> weights;
    std::vector<int> line_of;
    std::vector<const char*> tok;
    while (s < end) {
        const char* eol = (const char*)memchr(s, '\n', end - s);
        if (!eol) eol = end;
        ++line_no;
        tok.clear();
        std::vector<std::string> toks;
        for (const char* c = s; c < eol;) {
            while (c < eol && is_space(*c)) ++c;
            const char* b = c;
            while (c < eol && !is_space(*c)) ++c;
            if (c > b) toks.emplace_back(b, c);
        }
        s = eol + 1;
        auto to_int = [](const std::string& t, long* v) {
            char* e = nullptr;
            errno = 0;
            *v = strtol(t.c_str(), &e, 10);
            return e && *e == 0 && errno == 0 && *v >= INT32_MIN && *v <= INT32_MAX;
        };
        if (!have_header) {  // the first line: k L scoring weighting
            long h[4];
            if (toks.size() < 4 || !to_int(toks[0], &h[0]) || !to_int(toks[1], &h[1]) || !to_int(toks[2], &h[2]) || !to_int(toks[3], &h[3])) {
                set_error("vocabulary: %s line %d: bad header (expected k L scoring weighting)", path, line_no);
                return TC2LI_ERR_INVALID;
            }
            for (int i = 0; i < 4; ++i) hdr[i] = (int)h[i];
            have_header = true;
            continue;
        }
        if (toks.empty()) continue;
        if (toks.size() < 35) {
            set_error("vocabulary: %s line %d: %d fields, a node has 35 (parent, flag, 32 bytes, weight)", path, line_no, (int)toks.size());
            return TC2LI_ERR_INVALID;
        }
        long p, l, b;
        if (!to_int(toks[0], &p) || !to_int(toks[1], &l)) { set_error("vocabulary: %s line %d: bad parent or flag", path, line_no); return TC2LI_ERR_INVALID; }
        uint8_t d[32];
        for (int i = 0; i < 32; ++i) {
            if (!to_int(toks[2 + i], &b)) { set_error("vocabulary: %s line %d: bad descriptor byte", path, line_no); return TC2LI_ERR_INVALID; }
            d[i] = (uint8_t)(int)b;  // FORB::fromString: read as int, cast to unsigned char
        }
        char* e = nullptr;
        const double wt = strtod(toks[34].c_str(), &e);
        if (!e || *e != 0) { set_error("vocabulary: %s line %d: bad weight", path, line_no); return TC2LI_ERR_INVALID; }
        parent.push_back((int32_t)p); is_leaf.push_back((int32_t)l); desc.insert(desc.end(), d, d + 32); weights.push_back(wt);
        line_of.push_back(line_no);
    }
    if (!have_header) { set_error("vocabulary: %s: empty file", path); return TC2LI_ERR_INVALID; }
    const int rc = build_vocabulary(hdr[0], hdr[1], hdr[2], hdr[3], (int)parent.size(), parent.data(), is_leaf.data(), desc.data(), weights.data(),
                                    line_of.data(), out);
    if (rc < 0) { std::string m = std::string(path) + ": " + tc2li_last_error(); set_error("%s", m.c_str()); }
    return rc;
}

extern "C" int tc2li_vocabulary_info(const tc2li_vocabulary* v, int32_t* info) {
    if (!v || !info) { set_error("tc2li_vocabulary_info: invalid argument"); return TC2LI_ERR_INVALID; }
    info[0] = v->k; info[1] = v->L; info[2] = v->scoring; info[3] = v->weighting; info[4] = v->n_nodes(); info[5] = v->n_words;
    return 6;
}

extern "C" int tc2li_vocabulary_nodes(const tc2li_vocabulary* v, int32_t* parent, int32_t* word_id, uint8_t* descriptors, double* weights) {
    if (!v) { set_error("tc2li_vocabulary_nodes: invalid argument"); return TC2LI_ERR_INVALID; }
    const int n = v->n_nodes();
    if (parent) memcpy(parent, v->parent.data(), n * sizeof(int32_t));
    if (word_id) memcpy(word_id, v->word.data(), n * sizeof(int32_t));
    if (descriptors) memcpy(descriptors, v->desc.data(), (size_t)n * 32);
    if (weights) memcpy(weights, v->weight.data(), n * sizeof(double));
    return n;
}

extern "C" void tc2li_vocabulary_destroy(tc2li_vocabulary* v) { delete v; }

extern "C" int tc2li_vocabulary_transform_batch(tc2li_vocabulary* v, int n_frames, const uint8_t* descriptors, const int32_t* desc_offsets,
                                                int levelsup, const tc2li_bow_out* out, void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    if (!v || n_frames < 0 || !desc_offsets || !out_ok(out)) { set_error("tc2li_vocabulary_transform_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    std::vector<BowFrameDev> frames(n_frames);
    if (desc_offsets[0] != 0) { set_error("tc2li_vocabulary_transform_batch: desc_offsets[0] must be 0"); return TC2LI_ERR_INVALID; }
    for (int f = 0; f < n_frames; ++f) {
        if (desc_offsets[f + 1] < desc_offsets[f]) { set_error("tc2li_vocabulary_transform_batch: desc_offsets must not decrease"); return TC2LI_ERR_INVALID; }
        frames[f] = BowFrameDev{desc_offsets[f], desc_offsets[f], desc_offsets[f + 1] - desc_offsets[f], 0};
    }
    const size_t total = (size_t)desc_offsets[n_frames];
    if (total > 0 && !descriptors) { set_error("tc2li_vocabulary_transform_batch: descriptors is NULL"); return TC2LI_ERR_INVALID; }
    if (n_frames == 0) return 0;
    if (int rc = ensure_device(v)) return rc;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    return run_transform(v, nullptr, descriptors, frames, total, levelsup, out, st);
}

extern "C" int tc2li_orb_compute_bow_batch(tc2li_orb* o, tc2li_vocabulary* v, int n_frames, int levelsup, int capacity, const tc2li_bow_out* out,
                                           void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    if (!o || !v || n_frames < 0 || capacity < 0 || !out_ok(out)) { set_error("tc2li_orb_compute_bow_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    if (n_frames == 0) return 0;
    if (!orb_features_ready(o, n_frames, "tc2li_orb_compute_bow_batch")) return TC2LI_ERR_INVALID;
    std::vector<BowFrameDev> frames(n_frames);
    for (int f = 0; f < n_frames; ++f) {
        const int n = o->last_kp_cnt[2 * f];
        if (n > capacity) { set_error("tc2li_orb_compute_bow_batch: capacity %d < %d keypoints", capacity, n); return TC2LI_ERR_CAPACITY; }
        frames[f] = BowFrameDev{o->last_kp_off[2 * f], f * capacity, n, 0};
    }
    if (int rc = ensure_device(v)) return rc;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    return run_transform(v, o->d_desc.p, nullptr, frames, (size_t)n_frames * capacity, levelsup, out, st);
}

extern "C" int tc2li_search_by_bow_batch(const tc2li_bow_pair* pairs, int n_pairs, int capacity, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches,
                                         void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    if ((n_pairs > 0 && !pairs) || n_pairs < 0 || capacity < 0 || !kf_keypoint_of_keypoint || !n_matches) {
        set_error("tc2li_search_by_bow_batch: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    // the common nodes of every pair (both FeatureVectors ascending), the keypoint rows of the staged arrays
    std::vector<BowPairDev> P(n_pairs);
    std::vector<BowTaskDev> tasks;
    size_t n_keys = 0, n_idx = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const tc2li_keyframe_view& K = pairs[p].keyframe;
        const tc2li_keyframe_view& F = pairs[p].frame;
        if (K.n < 0 || F.n < 0 || K.n_nodes < 0 || F.n_nodes < 0 || (K.n > 0 && (!K.keys || !K.descriptors || !K.has_point)) ||
            (F.n > 0 && (!F.keys || !F.descriptors)) || (K.n_nodes > 0 && (!K.fv_node || !K.fv_offset || !K.fv_index)) ||
            (F.n_nodes > 0 && (!F.fv_node || !F.fv_offset || !F.fv_index))) {
            set_error("tc2li_search_by_bow_batch: pair %d has null arrays", p);
            return TC2LI_ERR_INVALID;
        }
        if (!feature_vector_ok(K) || !feature_vector_ok(F)) {
            set_error("tc2li_search_by_bow_batch: pair %d: a FeatureVector is malformed (fv_offset from 0 and not decreasing, fv_node strictly "
                      "ascending, fv_index in [0, n))", p);
            return TC2LI_ERR_INVALID;
        }
        if (F.n > capacity) { set_error("tc2li_search_by_bow_batch: capacity %d < %d keypoints of pair %d", capacity, F.n, p); return TC2LI_ERR_CAPACITY; }
        const int kf_idx = (int)n_idx, f_idx = kf_idx + (K.n_nodes ? K.fv_offset[K.n_nodes] : 0);
        P[p] = BowPairDev{(int32_t)n_keys, (int32_t)(n_keys + K.n), F.n, p * capacity, pairs[p].nn_ratio, pairs[p].check_orientation ? 1 : 0};
        for (int a = 0, b = 0; a < K.n_nodes && b < F.n_nodes;) {
            if (K.fv_node[a] == F.fv_node[b]) {
                BowTaskDev t{};
                t.pair = p;
                t.kf_pos = kf_idx + K.fv_offset[a]; t.kf_n = K.fv_offset[a + 1] - K.fv_offset[a];
                t.f_pos = f_idx + F.fv_offset[b]; t.f_n = F.fv_offset[b + 1] - F.fv_offset[b];
                if (t.f_n > 4096) { set_error("tc2li_search_by_bow_batch: pair %d node %d holds %d frame features (at most 4096)", p, F.fv_node[b], t.f_n); return TC2LI_ERR_CAPACITY; }
                if (t.kf_n > 0 && t.f_n > 0) tasks.push_back(t);
                ++a; ++b;
            } else if (K.fv_node[a] < F.fv_node[b]) ++a;
            else ++b;
        }
        n_keys += (size_t)K.n + F.n;
        n_idx += (size_t)(K.n_nodes ? K.fv_offset[K.n_nodes] : 0) + (F.n_nodes ? F.fv_offset[F.n_nodes] : 0);
    }
    if (n_pairs == 0) return 0;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    const size_t nk = std::max<size_t>(n_keys, 1), ni = std::max<size_t>(n_idx, 1), cap1 = std::max(capacity, 1);
    PackedTransfer T;
    const auto t_desc = T.io.take<OrbDescriptor>(nk);
    const auto t_ang = T.io.take<float>(nk);
    const auto t_hp = T.io.take<uint8_t>(nk);
    const auto t_idx = T.io.take<int32_t>(ni), t_match = T.work.take<int32_t>((size_t)n_pairs * cap1), t_nm = T.work.take<int32_t>(n_pairs);
    const auto t_pairs = T.io.take<BowPairDev>(n_pairs);
    const auto t_tasks = T.io.take<BowTaskDev>(std::max<size_t>(tasks.size(), 1));
    T.outputs_begin();
    TC2LI_HIP_CHECK(T.ensure(bws()));
    float* ang = T.host(t_ang);
    uint8_t* hp = T.host(t_hp);
    int32_t* fi = T.host(t_idx);
    size_t row = 0, idx = 0;  // the same running layout as above: per pair the keyframe, then the frame
    for (int p = 0; p < n_pairs; ++p) {
        for (int s = 0; s < 2; ++s) {
            const tc2li_keyframe_view& V = s ? pairs[p].frame : pairs[p].keyframe;
            T.io.put(t_desc, row, V.descriptors, V.n);
            for (int i = 0; i < V.n; ++i) {
                ang[row + i] = V.keys[i].angle;
                hp[row + i] = (s == 0 && V.has_point[i]) ? 1 : 0;
            }
            const int m = V.n_nodes ? V.fv_offset[V.n_nodes] : 0;
            for (int i = 0; i < m; ++i) {
                const int32_t x = V.fv_index[i];
                if (x < 0 || x >= V.n) { set_error("tc2li_search_by_bow_batch: pair %d: feature index %d out of range", p, x); return TC2LI_ERR_INVALID; }
                fi[idx + i] = x;
            }
            idx += m;
            row += V.n;
        }
    }
    T.io.put(t_pairs, 0, P.data(), n_pairs);
    T.io.put(t_tasks, 0, tasks.data(), tasks.size());
    TC2LI_HIP_CHECK(T.upload(st));
    int32_t *d_match = T.dev_work(t_match), *d_nm = T.dev_work(t_nm);
    TC2LI_HIP_CHECK(hipMemsetAsync(d_match, 0xff, (size_t)n_pairs * cap1 * sizeof(int32_t), st));
    launch_bow_search(T.dev(t_tasks), (int)tasks.size(), T.dev(t_pairs), n_pairs, T.dev(t_desc)->b, T.dev(t_ang), T.dev(t_hp), T.dev(t_idx), d_match, d_nm, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(kf_keypoint_of_keypoint, d_match, (size_t)n_pairs * capacity * 4, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_matches, d_nm, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return n_pairs;
}

// Tracking::TrackReferenceKeyFrame (SF/src/Tracking.cc:2603-2662), data path, for the frames of the last tc2li_orb_extract_batch call: the
// frame's ComputeBoW, ORBmatcher(0.7, true).SearchByBoW against the reference keyframe, the >= 15 branch, PoseOptimization from the last
// frame's pose, outlier discard and nmatchesMap -- one stream, one staging upload, the downloads of the results at the end.
extern "C" int tc2li_track_reference_keyframe_batch(tc2li_orb* o, tc2li_vocabulary* v, int n_frames, const tc2li_keypoint* keypoints,
                                                    const float* u_right, int capacity, const tc2li_reference_keyframe* refs,
                                                    const tc2li_camera* cam, double* poses7, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches,
                                                    int32_t* n_inliers, int32_t* n_matches_map, const tc2li_bow_out* bow, void* stream_) {
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;  // no CPU fallback: before anything else
    if (!o || !v || n_frames < 0 || capacity < 0 || !keypoints || !u_right || !refs || !cam || !poses7 || !kf_keypoint_of_keypoint || !n_matches ||
        !n_inliers || !n_matches_map || (bow && !out_ok(bow))) {
        set_error("tc2li_track_reference_keyframe_batch: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    if (n_frames == 0) return 0;
    if (!orb_features_ready(o, n_frames, "tc2li_track_reference_keyframe_batch")) return TC2LI_ERR_INVALID;
    if (o->prm.nlevels > kMaxLevels) { set_error("tc2li_track_reference_keyframe_batch: %d levels (at most %d)", o->prm.nlevels, kMaxLevels); return TC2LI_ERR_INVALID; }
    std::vector<BowFrameDev> frames(n_frames);
    std::vector<BowPairDev> P(n_frames);
    size_t nk = 0, ni = 0, nt = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int n = o->last_kp_cnt[2 * f];
        if (n > capacity) { set_error("tc2li_track_reference_keyframe_batch: capacity %d < %d keypoints", capacity, n); return TC2LI_ERR_CAPACITY; }
        if (n > 4096) { set_error("tc2li_track_reference_keyframe_batch: frame %d has %d keypoints (at most 4096)", f, n); return TC2LI_ERR_CAPACITY; }
        const tc2li_keyframe_view& K = refs[f].kf;
        if (K.n < 0 || K.n_nodes < 0 || (K.n > 0 && (!K.keys || !K.descriptors || !K.has_point || !refs[f].Xw || !refs[f].observed)) ||
            (K.n_nodes > 0 && (!K.fv_node || !K.fv_offset || !K.fv_index)) || !feature_vector_ok(K)) {
            set_error("tc2li_track_reference_keyframe_batch: reference keyframe %d has null arrays or a malformed FeatureVector", f);
            return TC2LI_ERR_INVALID;
        }
        frames[f] = BowFrameDev{o->last_kp_off[2 * f], f * capacity, n, 0};
        P[f] = BowPairDev{(int32_t)nk, o->last_kp_off[2 * f], n, f * capacity, 0.7f, 1};  // ORBmatcher matcher(0.7, true)
        nk += K.n;
        ni += K.n_nodes ? K.fv_offset[K.n_nodes] : 0;
        nt += K.n_nodes;
    }
    if (int rc = ensure_device(v)) return rc;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    const size_t nf = n_frames, ne = nf * std::max(capacity, 1);
    const size_t k1 = std::max<size_t>(nk, 1), i1 = std::max<size_t>(ni, 1), t1 = std::max<size_t>(nt, 1);
    // the upload block: the reference keyframes' arrays, their nodes as tasks, the pairs, the last poses, mvuRight and the transform's frame
    // records; device-only: the matches, the counts per frame, PoseOptimization's tables and the transform's
    PackedTransfer T;
    const auto t_desc = T.io.take<OrbDescriptor>(k1);
    const auto t_hp = T.io.take<uint8_t>(k1), t_obs = T.io.take<uint8_t>(k1);
    const auto t_ang = T.io.take<float>(k1), t_Xw = T.io.take<float>(3 * k1), t_pose = T.io.take<float>(7 * nf), t_ur = T.io.take<float>(ne);
    const auto t_idx = T.io.take<int32_t>(i1), t_node = T.io.take<int32_t>(t1);
    const auto t_tasks = T.io.take<BowTaskDev>(t1);
    const auto t_pairs = T.io.take<BowPairDev>(nf);
    const BowTransform B(T, n_frames, ne);  // Frame::ComputeBoW
    T.outputs_begin();
    const auto t_match = T.work.take<int32_t>(ne), t_nmatch = T.work.take<int32_t>(nf), t_ninl = T.work.take<int32_t>(nf), t_nmap = T.work.take<int32_t>(nf);
    const PoseTail pose(T.work, nf, ne);
    TC2LI_HIP_CHECK(T.ensure(bws()));
    float* ang = T.host(t_ang);
    uint8_t *hp = T.host(t_hp), *obs = T.host(t_obs);
    size_t row = 0, idx = 0;
    int n_tasks = 0;
    for (int f = 0; f < n_frames; ++f) {
        const tc2li_keyframe_view& K = refs[f].kf;
        T.io.put(t_desc, row, K.descriptors, K.n);
        T.io.put(t_Xw, 3 * row, refs[f].Xw, 3 * (size_t)K.n);
        for (int i = 0; i < K.n; ++i) {
            ang[row + i] = K.keys[i].angle;
            hp[row + i] = K.has_point[i] ? 1 : 0;
            obs[row + i] = refs[f].observed[i] ? 1 : 0;
        }
        for (int a = 0; a < K.n_nodes; ++a) {
            const int c = K.fv_offset[a + 1] - K.fv_offset[a];
            if (c == 0) continue;
            BowTaskDev t{};
            t.pair = f; t.kf_pos = (int32_t)idx + K.fv_offset[a]; t.kf_n = c;
            T.host(t_node)[n_tasks] = K.fv_node[a];
            T.host(t_tasks)[n_tasks++] = t;
        }
        const int m = K.n_nodes ? K.fv_offset[K.n_nodes] : 0;
        T.io.put(t_idx, idx, K.fv_index, m);
        T.io.put(t_pose, 7 * (size_t)f, refs[f].last_pose7, 7);
        idx += m;
        row += K.n;
    }
    T.io.put(t_pairs, 0, P.data(), nf);
    T.io.put(t_ur, 0, u_right, nf * capacity);
    T.io.put(B.frames, 0, frames.data(), nf);
    TC2LI_HIP_CHECK(T.upload(st));
    BowOutDev O;
    if (int rc = queue_transform(v, T, B, o->d_desc.p, 4, O, st)) return rc;  // levelsup 4
    auto W = [&](auto t) { return T.dev_work(t); };
    TC2LI_HIP_CHECK(hipMemsetAsync(W(t_match), 0xff, ne * sizeof(int32_t), st));
    BowRefArgs A{};
    A.n_frames = n_frames; A.n_tasks = n_tasks;
    A.tasks = T.dev(t_tasks); A.kf_node = T.dev(t_node); A.pairs = T.dev(t_pairs);
    A.kf_desc = T.dev(t_desc)->b; A.kf_has_point = T.dev(t_hp); A.kf_observed = T.dev(t_obs); A.kf_angle = T.dev(t_ang);
    A.kf_Xw = T.dev(t_Xw); A.kf_fv_index = T.dev(t_idx); A.last_pose7 = T.dev(t_pose);
    A.f_desc = o->d_desc.p; A.f_angle = o->d_angles.p; A.keys = o->d_mkeys.p; A.u_right = T.dev(t_ur);
    A.O = O;
    for (int l = 0; l < o->prm.nlevels; ++l) A.C.inv_sigma2[l] = o->inv_sigma2[l];
    A.match = W(t_match);
    A.n_matches = W(t_nmatch); A.inliers = W(pose.inliers); A.n_inliers = W(t_ninl); A.n_matches_map = W(t_nmap);
    A.probs = W(pose.probs); A.edges = W(pose.edges); A.Xw = W(pose.Xw); A.edge_kp = W(pose.edge_kp); A.poses = W(pose.poses); A.outlier = W(pose.outlier);
    launch_bow_reference(A, st);
    pose.launch(T, n_frames, cam, capacity, st);
    launch_bow_reference_finish(A, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(poses7, A.poses, 7 * nf * sizeof(double), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(kf_keypoint_of_keypoint, A.match, nf * capacity * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_matches, A.n_matches, nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_inliers, A.n_inliers, nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_matches_map, A.n_matches_map, nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (bow) { if (int rc = queue_transform_download(O, ne, n_frames, bow, st)) return rc; }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return n_frames;
}
