// A stand-alone driver for the host code of the covisibility graph on the map graph (tc2li_host_map_graph_update_connections,
// tc2li_host_map_graph_erase_connections and the validation they share with tc2li_map_graph_set_connections_batch), meant to be built
// with a sanitizer on the host side and run on a CPU: it makes no HIP call.  Build the library's sources and this file with
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -x hip -c <file>
// link them with hipcc -fsanitize=address,undefined into one program, and run it; it prints one line and returns 0.
// Random small graphs: every keyframe takes its turn as the current one, state to state, then every second keyframe is erased; tight
// capacities and broken tables are refused.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/tc2li_hip.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
};

struct Conn {
    std::vector<int32_t> co, ck, cw, oo, ok, ow;
    tc2li_map_graph_connections c{};
    void room(int rows, int nw, int no) {
        co.assign(rows + 1, 0); oo.assign(rows + 1, 0); ck.assign(nw, 0); cw.assign(nw, 0); ok.assign(no, 0); ow.assign(no, 0);   // exact: one entry more is a finding
        bind(rows);
    }
    void bind(int rows) {
        c.conn_offsets = co.data(); c.conn_kf = ck.data(); c.conn_weight = cw.data(); c.ord_offsets = oo.data(); c.ord_kf = ok.data(); c.ord_weight = ow.data();
        c.n_keyframes = rows;
    }
};

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "line %d: %s: %s\n", __LINE__, #cond, tc2li_last_error()); exit(1); } \
    } while (0)

}  // namespace

int main() {
    int updates = 0, erases = 0, refusals = 0;
    for (int seed = 1; seed <= 40; ++seed) {
        Rng r{(uint64_t)seed * 977};
        const int nk = 1 + r.below(seed < 30 ? 24 : 90), np = r.below(160);
        // the graph: every keyframe holds the points that it observes, and a few slots more
        std::vector<std::vector<int32_t>> obs(np), held(nk);
        for (int p = 0; p < np; ++p)
            for (int k = 0; k < nk; ++k)
                if (r.below(4) == 0) { obs[p].push_back(k); held[k].push_back(p); }
        std::vector<int32_t> kf_slot(nk, 0), slot_off(nk + 1, 0), slot_point, obs_off(np + 1, 0), obs_kf, obs_index;
        std::vector<int64_t> kf_id(nk);
        std::vector<uint8_t> kf_flags(nk), point_flags(np + 1);
        std::vector<double> poses7(7 * (size_t)nk + 1, 0.0), positions(3 * (size_t)np + 1, 0.0);
        for (int k = 0; k < nk; ++k) {
            kf_id[k] = 100 + k; kf_flags[k] = (uint8_t)(r.below(12) == 0 ? 1 + r.below(2) : 0) | (uint8_t)(r.below(2) << 2);
            for (int32_t p : held[k]) { slot_point.push_back(p); if (r.below(9) == 0) slot_point.push_back(r.below(3) ? p : -1); }
            slot_off[k + 1] = (int32_t)slot_point.size();
        }
        for (int p = 0; p < np; ++p) {
            point_flags[p] = (uint8_t)((r.below(15) == 0 ? 1 : 0) | (r.below(2) << 1));
            for (int32_t k : obs[p]) { obs_kf.push_back(k); obs_index.push_back(-1); }
            obs_off[p + 1] = (int32_t)obs_kf.size();
        }
        tc2li_map_graph_tables t{};
        t.kf_slot = kf_slot.data(); t.kf_id = kf_id.data(); t.kf_flags = kf_flags.data(); t.poses7 = poses7.data(); t.slot_offsets = slot_off.data();
        t.slot_point = slot_point.data(); t.point_flags = point_flags.data(); t.positions = positions.data(); t.obs_offsets = obs_off.data();
        t.obs_kf = obs_kf.data(); t.obs_index = obs_index.data(); t.n_keyframes = nk; t.n_points = np;
        // connections that cover the first rows only: the rest were "appended since"
        Conn now;
        now.room(nk - nk / 3, 0, 0);
        int32_t sizes[2], counts[TC2LI_CONNECTIONS_COUNTS];
        for (int turn = 0; turn < nk + 4; ++turn) {
            const int cur = turn < nk ? (turn * 7) % nk : r.below(nk);
            Conn probe, next;
            probe.room(nk, 0, 0);
            const int32_t none[2] = {0, 0};
            int rc = tc2li_host_map_graph_update_connections(&t, &now.c, cur, turn & 1, 100 + r.below(nk), &probe.c, none, sizes, counts);
            if (rc == TC2LI_ERR_CAPACITY) ++refusals; else CHECK(rc >= 0 && sizes[0] == 0 && sizes[1] == 0);
            next.room(nk, sizes[0], sizes[1]);
            const int32_t caps[2] = {sizes[0], sizes[1]};
            rc = tc2li_host_map_graph_update_connections(&t, &now.c, cur, turn & 1, 100 + cur * (turn & 2 ? 1 : 0), &next.c, caps, sizes, counts);
            CHECK(rc == counts[TC2LI_CONNECTIONS_STATUS] && next.c.n_keyframes == nk && next.co[nk] == sizes[0] && next.oo[nk] == sizes[1]);
            now = next; now.bind(nk);
            ++updates;
        }
        for (int row = 0; row < nk; row += 2) {
            Conn probe, next;
            probe.room(nk, 0, 0);
            const int32_t none[2] = {0, 0};
            if (tc2li_host_map_graph_erase_connections(&t, &now.c, row, &probe.c, none, sizes) == TC2LI_ERR_CAPACITY) ++refusals;
            next.room(nk, sizes[0], sizes[1]);                                       // a list rebuilt from the whole weight row may be longer than the one it replaces
            const int32_t caps[2] = {sizes[0], sizes[1]};
            CHECK(tc2li_host_map_graph_erase_connections(&t, &now.c, row, &next.c, caps, sizes) == 0);
            CHECK(next.co[row + 1] == next.co[row] && next.oo[row + 1] == next.oo[row] && sizes[0] <= caps[0]);
            for (int k = 0; k < nk; ++k)                                             // (a keyframe outside the row's own weights may still name it: the maps are not symmetric)
                for (int j = now.co[row]; j < now.co[row + 1]; ++j)
                    if (now.ck[j] == k)
                        for (int i = next.co[k]; i < next.co[k + 1]; ++i) CHECK(next.ck[i] != row);
            now = next; now.bind(nk);
            ++erases;
        }
        // broken tables are refused and nothing is written
        if (now.co[nk] > 0) {
            Conn bad = now, out;
            bad.bind(nk);
            out.room(nk, now.co[nk], now.oo[nk] + now.co[nk]);
            const int32_t caps[2] = {now.co[nk], now.oo[nk] + now.co[nk]};
            int first = 0;
            while (bad.co[first + 1] == bad.co[first]) ++first;
            bad.ck[bad.co[first]] = first;                                           // its own keyframe
            CHECK(tc2li_host_map_graph_erase_connections(&t, &bad.c, 0, &out.c, caps, sizes) == TC2LI_ERR_INVALID);
            bad.ck[bad.co[first]] = nk;                                              // out of range
            CHECK(tc2li_host_map_graph_erase_connections(&t, &bad.c, 0, &out.c, caps, sizes) == TC2LI_ERR_INVALID);
            bad = now; bad.bind(nk);
            bad.co[1] = bad.co[0] - 1;                                               // offsets that fall
            CHECK(tc2li_host_map_graph_erase_connections(&t, &bad.c, 0, &out.c, caps, sizes) == TC2LI_ERR_INVALID);
            CHECK(tc2li_host_map_graph_erase_connections(&t, &now.c, nk, &out.c, caps, sizes) == TC2LI_ERR_INVALID);
            refusals += 4;
        }
    }
    printf("map graph connections, host code: %d updates, %d erases, %d refusals\n", updates, erases, refusals);
    return 0;
}
