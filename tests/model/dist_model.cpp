/*
 * tests/model/dist_model.cpp -- TEST INFRASTRUCTURE: an independent reference for the edge list of
 * the outcome distribution (include/dsm.h, dsm_reach_dist*).  It reuses the state, the round and
 * the canonical words of tests/model/reach_model.cpp (the oracle's handler orc_step, one action at
 * a time; nothing of dsm_table.h, dsm_reach.h or dsm_dist.h) and runs a breadth-first search of
 * its own that keeps every edge: states are told apart by their full canonical words, never by
 * a fingerprint, so an edge that the library's fingerprint look-up sent to a wrong state would
 * show.  Numbering and limits are the search's: levels in order, parents ascending, masks
 * ascending; a level that would pass max_states is dropped whole, with its edges; no level
 * deeper than max_depth.
 *
 *   dist_model <np> <stride> <traces.u16> <counts.u32> <inbox_limit> <max_states> <max_depth> <out_prefix>
 * writes <out_prefix>.edges (u32 quadruples: source, target, k = |A(source)|, m = popcount(mask),
 * sources ascending, masks ascending) and <out_prefix>.cls (u8 per state: 0 running and expanded,
 * 1 running in the unexpanded last level of a cut search, 2 + status for a terminal state).
 * tests/test_dist_host.py pushes the mass over that list with Python integers.
 */
#define main reach_model_main
#include "reach_model.cpp"
#undef main

namespace {

int dist(uint64_t max_states, uint32_t max_depth, const char *prefix) {
    std::vector<State> S(1);
    std::map<std::vector<uint32_t>, uint64_t> seen;
    std::vector<uint32_t> edges;
    root(S[0]);
    seen[words(S[0])] = 0;
    uint64_t lo = 0, hi = 1, n_exp = 0;
    bool cut = false;
    for (uint32_t depth = 0;; ++depth) {
        uint64_t total = 0;
        for (uint64_t p = lo; p < hi; ++p) {
            const uint32_t a = enabled(S[p]);
            if (a) total += (1u << __builtin_popcount(a)) - 1u;
        }
        if (total == 0) break;
        if ((max_depth && depth >= max_depth) || depth + 1 >= MAX_LEVELS) { cut = true; break; }
        const size_t edges_before = edges.size();
        bool over = false;
        for (uint64_t p = lo; p < hi && !over; ++p) {
            const uint32_t a = enabled(S[p]);
            const uint32_t k = (uint32_t)__builtin_popcount(a), cnt = a ? (1u << k) - 1u : 0u;
            for (uint32_t j = 1; j <= cnt && !over; ++j) {
                const uint32_t mask = deposit(j, a);
                State x = S[p];
                round_of(x, mask);
                const std::vector<uint32_t> w = words(x);
                uint64_t id;
                const auto it = seen.find(w);
                if (it != seen.end()) {
                    id = it->second;
                } else {
                    id = S.size();
                    if (id >= max_states) { over = true; break; }
                    seen[w] = id;
                    S.push_back(x);
                }
                const uint32_t e[4] = {(uint32_t)p, (uint32_t)id, k, (uint32_t)__builtin_popcount(mask)};
                edges.insert(edges.end(), e, e + 4);
            }
        }
        if (over) {                                              /* the level is dropped whole */
            S.resize(hi);
            edges.resize(edges_before);
            cut = true;
            break;
        }
        n_exp = hi;
        if (S.size() == hi) break;
        lo = hi;
        hi = S.size();
    }
    if (!cut) n_exp = S.size();
    std::vector<uint8_t> cls(S.size());
    for (uint64_t p = 0; p < S.size(); ++p) {
        if (enabled(S[p])) cls[p] = p < n_exp ? 0 : 1;
        else cls[p] = (uint8_t)(2u + (result(S[p]).status & 0xFFu));
    }
    return dumpf(prefix, ".edges", edges.data(), edges.size() * 4) && dumpf(prefix, ".cls", cls.data(), cls.size()) ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: dist_model np stride traces counts inbox_limit max_states max_depth out_prefix\n");
        return 2;
    }
    g_np = atoi(argv[1]);
    g_stride = (uint32_t)strtoul(argv[2], 0, 0);
    g_limit = (uint32_t)strtoul(argv[5], 0, 0);
    if ((g_np != 4 && g_np != 8) || !g_stride || !g_limit || g_limit > 16) return 2;
    g_trace = (const uint16_t *)slurp(argv[3], (size_t)g_np * g_stride * 2);
    g_counts = (const uint32_t *)slurp(argv[4], (size_t)g_np * 4);
    if (!g_trace || !g_counts) { fprintf(stderr, "dist_model: cannot read the inputs\n"); return 1; }
    return dist(strtoull(argv[6], 0, 0), (uint32_t)strtoul(argv[7], 0, 0), argv[8]);
}
