// tc2li_inertial_term_batch / tc2li_host_inertial_term_batch / tc2li_inertial_term_limits (include/tc2li_hip.h "the inertial term of
// local-BA windows"): the inertial edges of many windows evaluated at given states -- robust cost and, when asked, the normal equations in
// blocks of 15 unknowns per keyframe.  This file validates the windows, prepares what the reference computes once per edge on the host
// (EdgeInertial's information with its eigenvalue clamp and the random-walk informations: InertialLinkHost::prepare), concatenates the
// windows into the tables of inertial_term_device.hpp, and either sends them through inertial_term_kernels.hip or runs the same per-link
// function and the same link-order sums on the tracking pool.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "inertial_host.hpp"
#include "inertial_term_device.hpp"
#include "packed_batch.hpp"

static_assert(sizeof(tc2li_inertial_term_problem) == 72, "ABI layout");

namespace tc2li {
namespace {

// What both entries make of the problems: the concatenated tables
struct ItTables {
    std::vector<PiState> states;
    std::vector<PiPreint> pre;
    std::vector<ItLink> links;
    std::vector<int32_t> kf_off, kf_items, win_link_off, win_kf_off;
    double huber_d = 0;
    float huber_dsqr = 0;
};

std::string check_window(const tc2li_inertial_term_problem& in, bool linearize) {
    char text[160];
    if (in.n_keyframes < 0 || in.n_links < 0) return "negative size";
    if (in.n_keyframes > kItMaxKeyframes || in.n_links > kItMaxLinks) {
        snprintf(text, sizeof(text), "%d keyframes and %d links are beyond the limits of %d and %d", in.n_keyframes, in.n_links, kItMaxKeyframes, kItMaxLinks);
        return text;
    }
    if (!in.chi2) return "null chi2";
    if (in.n_keyframes && (!in.keyframes || !in.fixed || !in.has_imu)) return "null keyframes, fixed or has_imu";
    if (in.n_links && !in.links) return "null links";
    if (linearize && ((in.n_keyframes && (!in.H_diag || !in.b)) || (in.n_links && !in.H_link))) return "null H_diag, H_link or b";
    for (int l = 0; l < in.n_links; ++l) {
        const tc2li_inertial_link& lk = in.links[l];
        const char* what = nullptr;
        if (lk.kf1 < 0 || lk.kf1 >= in.n_keyframes || lk.kf2 < 0 || lk.kf2 >= in.n_keyframes) what = "keyframe index out of range";
        else if (lk.kf1 == lk.kf2) what = "kf1 == kf2";
        else if (!in.has_imu[lk.kf1] || !in.has_imu[lk.kf2]) what = "joins a keyframe without IMU state";
        else if (!lk.preintegrated) what = "null pre-integration";
        if (what) {
            snprintf(text, sizeof(text), "link %d: %s", l, what);
            return text;
        }
    }
    return "";
}

// Validation and the tables.  TC2LI_OK, or the error's code with the error set; nothing of the problems is written.
int prepare(const char* entry, const tc2li_inertial_term_problem* problems, int n_problems, bool linearize, ItTables& T) {
    if (n_problems < 0 || (n_problems > 0 && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    std::vector<std::string> found(n_problems);
    const int rc = validate_each(entry, "window", n_problems, [&](int p, const char** what) {
        found[p] = check_window(problems[p], linearize);
        *what = found[p].c_str();
        return found[p].empty() ? 0 : TC2LI_ERR_INVALID;
    });
    if (rc) return rc;
    T.win_link_off.assign(n_problems + 1, 0);
    T.win_kf_off.assign(n_problems + 1, 0);
    size_t n_kf = 0, n_links = 0;
    for (int p = 0; p < n_problems; ++p) {
        n_kf += (size_t)problems[p].n_keyframes; n_links += (size_t)problems[p].n_links;
        if (n_kf > kMaxRows / kItBlock || n_links > kMaxRows / kItPerLink) return too_many_rows(entry, p);
        T.win_kf_off[p + 1] = (int32_t)n_kf; T.win_link_off[p + 1] = (int32_t)n_links;
    }
    T.states.resize(n_kf); T.pre.resize(n_links); T.links.resize(n_links);
    std::vector<int32_t> link_window(n_links);
    T.kf_off.assign(n_kf + 1, 0);
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_term_problem& in = problems[p];
        const int32_t k0 = T.win_kf_off[p], l0 = T.win_link_off[p];
        for (int k = 0; k < in.n_keyframes; ++k) pi_state_from(in.keyframes[k], T.states[k0 + k]);
        for (int l = 0; l < in.n_links; ++l) {
            const tc2li_inertial_link& lk = in.links[l];
            const int free_mask = (in.fixed[lk.kf1] ? 0 : 1) | (in.fixed[lk.kf2] ? 0 : 2);
            T.links[l0 + l] = ItLink{k0 + lk.kf1, k0 + lk.kf2, lk.robust ? 1 : 0, free_mask};
            link_window[l0 + l] = p;
            if (free_mask & 1) ++T.kf_off[k0 + lk.kf1 + 1];
            if (free_mask & 2) ++T.kf_off[k0 + lk.kf2 + 1];
        }
    }
    // per keyframe the links that have it as a free end, in link order
    for (size_t k = 0; k < n_kf; ++k) T.kf_off[k + 1] += T.kf_off[k];
    T.kf_items.resize(T.kf_off[n_kf]);
    {
        std::vector<int32_t> at(T.kf_off.begin(), T.kf_off.end() - 1);
        for (size_t l = 0; l < n_links; ++l) {
            const ItLink& lk = T.links[l];
            if (lk.free_mask & 1) T.kf_items[at[lk.kf1]++] = (int32_t)(l << 1);
            if (lk.free_mask & 2) T.kf_items[at[lk.kf2]++] = (int32_t)(l << 1 | 1);
        }
    }
    // the informations, once per link and call
    std::vector<uint8_t> bad(n_links, 0);
    tracking_pool().parallel_for((int)n_links, [&](int l) {
        const int p = link_window[l];
        const tc2li_inertial_link& in = problems[p].links[l - T.win_link_off[p]];
        InertialLinkHost h;
        h.pre = in.preintegrated;
        if (!h.prepare(in.info_scale)) { bad[l] = 1; return; }
        PiPreint& d = T.pre[l];
        memset(&d, 0, sizeof(d));
        pi_preint_from(*in.preintegrated, d);
        memcpy(d.info, h.info, sizeof(h.info)); memcpy(d.infoG, h.infoG, sizeof(h.infoG)); memcpy(d.infoA, h.infoA, sizeof(h.infoA));
    });
    for (size_t l = 0; l < n_links; ++l)
        if (bad[l]) {
            const int p = link_window[l];
            set_error("%s: window %d: link %d: the pre-integration covariance is not positive definite", entry, p, (int)l - T.win_link_off[p]);
            return TC2LI_ERR_INVALID;
        }
    const float d_imu = sqrtf(16.92f);  // as InertialTerm::prepare
    T.huber_d = d_imu;
    T.huber_dsqr = (float)((double)d_imu * (double)d_imu);
    return TC2LI_OK;
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_inertial_term_limits(int32_t* out, int capacity) {
    if (!out || capacity < 2) {
        set_error("tc2li_inertial_term_limits: room for 2 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kItMaxKeyframes; out[1] = kItMaxLinks;
    return 2;
}

extern "C" int tc2li_host_inertial_term_batch(const tc2li_inertial_term_problem* problems, int n_problems, int linearize) {
    ItTables T;
    const int rc = prepare("tc2li_host_inertial_term_batch", problems, n_problems, linearize != 0, T);
    if (rc < 0) return rc;
    const size_t n_links = T.links.size();
    std::vector<double> cost(n_links), blocks(linearize ? n_links * kItPerLink : 0);
    std::vector<double*> link_out(n_links, nullptr);
    if (linearize)
        for (int p = 0; p < n_problems; ++p)
            for (int l = 0; l < problems[p].n_links; ++l) link_out[T.win_link_off[p] + l] = problems[p].H_link + (size_t)l * kItBlock;
    tracking_pool().parallel_for((int)n_links, [&](int l) {
        const ItLink& lk = T.links[l];
        ItVals v;
        double J[216], W[216];
        double* const side1 = linearize ? blocks.data() + (size_t)l * kItPerLink : nullptr;
        it_link(T.pre[l], T.states[lk.kf1], T.states[lk.kf2], lk, T.huber_d, T.huber_dsqr, linearize != 0, v, J, W, side1, side1 ? side1 + kItSide : nullptr,
                link_out[l], 0, 1, ItNoSync());
        cost[l] = it_cost(v);
    });
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_inertial_term_problem& in = problems[p];
        in.chi2[0] = it_window_chi2(cost.data(), T.win_link_off[p], T.win_link_off[p + 1]);
        if (!linearize) return;
        for (int k = 0; k < in.n_keyframes; ++k) {
            const int kf = T.win_kf_off[p] + k;
            for (int e = 0; e < kItSide; ++e) {
                const double s = it_keyframe_entry(T.kf_items.data(), T.kf_off[kf], T.kf_off[kf + 1], blocks.data(), e);
                if (e < kItBlock) in.H_diag[(size_t)k * kItBlock + e] = s;
                else in.b[(size_t)k * kItU + (e - kItBlock)] = s;
            }
        }
    });
    return n_problems;
}

extern "C" int tc2li_inertial_term_batch(const tc2li_inertial_term_problem* problems, int n_problems, int linearize, void* stream) {
    const char* entry = "tc2li_inertial_term_batch";
    ItTables H;
    const int rc = prepare(entry, problems, n_problems, linearize != 0, H);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    const size_t np = (size_t)n_problems, n_links = H.links.size(), n_kf = H.states.size(), n_items = H.kf_items.size();
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const size_t o_state = io.take(n_kf * sizeof(PiState)), o_pre = io.take(n_links * sizeof(PiPreint)), o_link = io.take(n_links * sizeof(ItLink)),
                 o_koff = io.take((n_kf + 1) * 4), o_item = io.take(n_items * 4), o_woff = io.take((np + 1) * 4);
    T.outputs_begin();
    const size_t o_chi2 = io.take(np * 8);
    const size_t o_hd = linearize ? io.take(n_kf * kItBlock * 8) : 0, o_hl = linearize ? io.take(n_links * kItBlock * 8) : 0,
                 o_b = linearize ? io.take(n_kf * kItU * 8) : 0;
    const size_t o_cost = work.take(n_links * 8), o_blocks = linearize ? work.take(n_links * kItPerLink * 8) : 0;
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceInertialTerm>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_state, 0, H.states.data(), n_kf, sizeof(PiState));
    io.put(o_pre, 0, H.pre.data(), n_links, sizeof(PiPreint));
    io.put(o_link, 0, H.links.data(), n_links, sizeof(ItLink));
    io.put(o_koff, 0, H.kf_off.data(), n_kf + 1, 4);
    io.put(o_item, 0, H.kf_items.data(), n_items, 4);
    io.put(o_woff, 0, H.win_link_off.data(), np + 1, 4);
    TC2LI_HIP_CHECK(T.upload(st));
    ItBatch B{};
    B.states = T.dev<PiState>(o_state); B.pre = T.dev<PiPreint>(o_pre); B.links = T.dev<ItLink>(o_link);
    B.kf_off = T.dev<int32_t>(o_koff); B.kf_items = T.dev<int32_t>(o_item); B.win_link_off = T.dev<int32_t>(o_woff);
    B.chi2 = T.dev<double>(o_chi2);
    if (linearize) { B.H_diag = T.dev<double>(o_hd); B.H_link = T.dev<double>(o_hl); B.b = T.dev<double>(o_b); B.blocks = T.dev_work<double>(o_blocks); }
    B.cost = T.dev_work<double>(o_cost);
    B.n_links = (int32_t)n_links; B.n_keyframes = (int32_t)n_kf; B.n_windows = n_problems;
    B.huber_d = H.huber_d; B.huber_dsqr = H.huber_dsqr;
    launch_inertial_term(B, linearize != 0, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_term_problem& in = problems[p];
        io.get(in.chi2, o_chi2, (size_t)p, 1, 8);
        if (!linearize) continue;
        io.get(in.H_diag, o_hd, (size_t)H.win_kf_off[p], (size_t)in.n_keyframes, kItBlock * 8);
        io.get(in.H_link, o_hl, (size_t)H.win_link_off[p], (size_t)in.n_links, kItBlock * 8);
        io.get(in.b, o_b, (size_t)H.win_kf_off[p], (size_t)in.n_keyframes, kItU * 8);
    }
    return n_problems;
}
