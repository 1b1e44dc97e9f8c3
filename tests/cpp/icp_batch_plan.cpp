// icp_batch_plan.cpp -- dumps lm_host.cpp's plan of an ICP refinement (plan_icp_batch, plan_icp_levels) for a query
// list given on the command line, for tests/test_icp_batch_plan_cpu.py to check.  Host code alone: g++, no HIP.
// usage: icp_batch_plan <step> <iterations> <levels> <tolerance> <budget bytes> <npx,nm,first_pose,np,rows> ...
//        rows = the scene cloud's rows of the query once they are known (negative: the query is not refined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lm_host.h"

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: see the file head\n"); return 2; }
    const int step = std::atoi(argv[1]), iterations = std::atoi(argv[2]), levels = std::atoi(argv[3]);
    const double tolerance = std::atof(argv[4]);
    const size_t budget = (size_t)std::strtoull(argv[5], nullptr, 10);
    std::vector<lmh::IcpQueryIn> q;
    std::vector<int> rows;
    for (int a = 6; a < argc; ++a) {
        lmh::IcpQueryIn e;
        int r = 0;
        if (std::sscanf(argv[a], "%d,%d,%d,%d,%d", &e.npx, &e.nm, &e.first_pose, &e.np, &r) != 5) { std::fprintf(stderr, "bad query %s\n", argv[a]); return 2; }
        q.push_back(e);
        rows.push_back(r);
    }
    lmh::IcpBatchPlan plan;
    lmh::plan_icp_batch(q, step, levels, budget, plan);
    for (size_t ci = 0; ci < plan.chunks.size(); ++ci) {
        const lmh::IcpChunkPlan& c = plan.chunks[ci];
        std::printf("chunk %zu bytes %zu np %d nlevels %d g_px %u g_normals %u\n", ci, c.bytes, c.np, c.nlevels, c.g_px, c.g_normals);
        for (const lmh::IcpRegion& r : c.regions()) std::printf("region %s %d %zu %zu\n", r.name, r.query, r.off, r.bytes);
        std::vector<int> crow;
        for (const lmh::IcpQueryPlan& e : c.q) {
            std::printf("query %d npx %d nb %d nm %d np %d ns_cap %d nch_cap %d nblk_cap %d\n", e.query, e.npx, e.nb, e.nm, e.np, e.ns_cap, e.nch_cap,
                        e.nblk_cap);
            crow.push_back(rows[(size_t)e.query]);
        }
        lmh::IcpLevelsPlan lp;
        lmh::plan_icp_levels(c, crow, iterations, levels, tolerance, lp);
        std::printf("poses %d\n", lp.np);
        for (size_t k = 0; k < c.q.size(); ++k) {
            std::printf("pose0 %d %d\n", c.q[k].query, lp.pose0[k]);
            for (int l = 0; l < lp.nlevels; ++l) {
                const LmIcpLevel& L = lp.lev[k * (size_t)lp.nlevels + (size_t)l];
                std::printf("lev %d %d level %d s %d nL %d ndL %d rounds %d max_it %d tolp %.17g\n", c.q[k].query, l, L.level, L.s, L.nL, L.ndL, L.rounds,
                            L.max_it, L.tolp);
            }
        }
        for (int l = 0; l < lp.nlevels; ++l) {
            const lmh::IcpLevelLaunch& g = lp.level[(size_t)l];
            std::printf("launch %d rounds %d g_src %u g_chunks %u g_dst %u\n", l, g.rounds, g.g_src, g.g_chunks, g.g_dst);
        }
    }
    std::printf("OK %zu\n", plan.chunks.size());
    return 0;
}
