// projection_search.hpp: what is not inline.
#include "projection_search.hpp"

#include <algorithm>
#include <cstdlib>

namespace tc2li {

int SearchScratch::ensure(int n_frames, int total_q, int capacity) {
    const char* per_query = getenv("TC2LI_MATCH_POOL_PER_QUERY");  // tests shrink the pool to reach the overflow path
    const size_t nq = (size_t)std::max(total_q, 1), nf = (size_t)std::max(n_frames, 1);
    pool_cap = std::max(1, per_query ? atoi(per_query) : 32) * (int)nq;
    TC2LI_HIP_CHECK(d_queries.ensure(nq));
    for (DevBuf<int32_t>* b : {&d_query_frame, &d_match, &d_prev, &d_cand_off, &d_cand_cnt, &d_amb_ids, &d_amb_level}) TC2LI_HIP_CHECK(b->ensure(nq));
    TC2LI_HIP_CHECK(d_amb_ratio.ensure(nq)); TC2LI_HIP_CHECK(d_amb_r.ensure(nq));
    TC2LI_HIP_CHECK(d_rounds.ensure(nf)); TC2LI_HIP_CHECK(d_nmatch.ensure(nf));
    TC2LI_HIP_CHECK(d_cell_start.ensure(nf * kCellsPlus1)); TC2LI_HIP_CHECK(d_small.ensure(4));
    TC2LI_HIP_CHECK(d_items.ensure(nf * std::max(capacity, 1))); TC2LI_HIP_CHECK(d_pool.ensure(pool_cap));
    TC2LI_HIP_CHECK(h_small.ensure(4)); TC2LI_HIP_CHECK(h_amb_level.ensure(nq)); TC2LI_HIP_CHECK(h_amb_ratio.ensure(nq));
    return TC2LI_OK;
}

int resolve_ambiguous_levels(SearchScratch& s, const TrackConst& C, PatchLauncher patch, hipStream_t st) {
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(s.h_small.p + 2, s.amb_count(), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    const int n_amb = s.h_small.p[2];
    if (n_amb <= 0) return TC2LI_OK;
    TC2LI_HIP_CHECK(hipMemcpyAsync(s.h_amb_ratio.p, s.d_amb_ratio.p, n_amb * sizeof(float), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    const int chunk = 16384, n_chunks = (n_amb + chunk - 1) / chunk;  // one chunk runs on the calling thread
    tracking_pool().parallel_for(n_chunks, [&](int c) {
        const int k1 = std::min(n_amb, (c + 1) * chunk);
        for (int k = c * chunk; k < k1; ++k) s.h_amb_level.p[k] = predict_scale_level(s.h_amb_ratio.p[k], C.log_scale, C.n_levels);
    });
    TC2LI_HIP_CHECK(hipMemcpyAsync(s.d_amb_level.p, s.h_amb_level.p, n_amb * sizeof(int32_t), hipMemcpyHostToDevice, st));
    patch(s.d_amb_ids.p, s.d_amb_level.p, s.d_amb_r.p, n_amb, C, s.d_queries.p, st);
    return TC2LI_OK;
}

int frame_grids(tc2li_orb* o, hipStream_t st, FrameGrids* out) {
    *out = FrameGrids{};
    const char* cache = getenv("TC2LI_MATCH_GRID_CACHE");  // read per call: 0 = every search builds its own grids (the A/B runs, a test)
    if (cache && atoi(cache) == 0) return TC2LI_OK;
    const int nf = o->last_nimg / 2;
    if (nf <= 0) return TC2LI_OK;
    std::lock_guard<std::mutex> lk(o->grid_mutex);
    if (!o->grid_valid) {
        PackedTransfer T;
        const Table<MatchFrameDev> frames = T.io.take<MatchFrameDev>(nf);
        const Table<int32_t> key_base = T.io.take<int32_t>(nf);
        T.outputs_begin();
        TC2LI_HIP_CHECK(o->d_grid_cells.ensure((size_t)nf * kCellsPlus1)); TC2LI_HIP_CHECK(o->d_grid_items.ensure(o->d_mkeys.n));
        TC2LI_HIP_CHECK(T.ensure(o->grid_tab));
        if (!o->grid_event) TC2LI_HIP_CHECK(hipEventCreateWithFlags(&o->grid_event, hipEventDisableTiming));
        for (int f = 0; f < nf; ++f) {
            const int off = o->last_kp_off[2 * f], n = o->last_kp_cnt[2 * f];
            // a frame with more keys than the matcher takes is refused by every search (check_match_keys): its grid stays empty
            T.host(frames)[f] = MatchFrameDev{o->d_mkeys.p + off, nullptr, nullptr, nullptr, nullptr, n <= kMaxMatchKeys ? n : 0, 0, 0, 0,
                                              0.0f, (float)o->cur_w, 0.0f, (float)o->cur_h};
            T.host(key_base)[f] = off;
        }
        TC2LI_HIP_CHECK(T.upload(st));
        MatchLists L{};
        L.cell_start = o->d_grid_cells.p; L.items = o->d_grid_items.p; L.key_base = T.dev(key_base);
        launch_match_grid(T.dev(frames), nf, L, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipEventRecord(o->grid_event, st));
        o->grid_valid = true; o->grid_stream = st; ++o->grid_builds;
    } else if (st != o->grid_stream) {
        TC2LI_HIP_CHECK(hipStreamWaitEvent(st, o->grid_event, 0));
    }
    out->cell_start = o->d_grid_cells.p; out->items = o->d_grid_items.p;
    return TC2LI_OK;
}

int projection_search(SearchScratch& s, const SearchPass& P, hipStream_t st, const std::function<int()>& behind) {
    const bool cached = P.grid_cells != nullptr;
    const MatchLists L{cached ? P.grid_cells : s.d_cell_start.p, cached ? P.grid_items : s.d_items.p, P.d_key_base, s.d_cand_off.p, s.d_cand_cnt.p,
                       s.d_pool.p, s.pool_top(), s.pool_cap, cached ? 1 : 0, cached ? P.d_cell_row : nullptr};
    launch_match_lists(P.d_mframes, P.n_pass, s.d_query_frame.p, P.total_q, L, P.mode, P.nn_ratio, s.d_match.p, s.d_prev.p, s.d_rounds.p, st, P.orb_dist);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(s.h_small.p, s.pool_top(), 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (behind) { if (int rc = behind()) return rc; }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    if (!s.h_small.p[1]) return TC2LI_OK;
    // candidate pool exhausted (very dense windows).  The query kernels reset the matches when they build the queries; here it is due alone.
    for (int k = 0; k < P.n_pass; ++k) {
        const TrackFrameDev& F = P.h_frames[P.h_pass ? P.h_pass[k] : k];
        if (F.n_q) TC2LI_HIP_CHECK(hipMemsetAsync(s.d_match.p + F.q_off, 0xff, (size_t)F.n_q * sizeof(int32_t), st));
    }
    launch_match_by_projection(P.d_mframes, P.n_pass, P.mode, P.nn_ratio, s.d_match.p, s.d_prev.p, s.d_rounds.p, st, P.orb_dist);
    TC2LI_HIP_CHECK(hipGetLastError());
    if (!behind) return TC2LI_OK;
    if (int rc = behind()) return rc;
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    return TC2LI_OK;
}

}  // namespace tc2li
