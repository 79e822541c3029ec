// plan_driver — the host plan of a graph upload (visfs_amd/csrc/ba_plan.hpp) on its own, without HIP: reads one graph and the
// decisions of an upload, runs the summary and the plan, prints every array and scalar of the plan.  tests/test_upload_plan.py compares
// the printout with an independent statement of the same structure (tests/upload_plan_oracle.py).
//   g++ -std=c++17 -O2 -pthread -I include -I visfs_amd/csrc tests/cpp/plan_driver.cpp -o plan_driver;  plan_driver < graph.txt
// Input and output: lines of `name count value ...`.
#include <cstdio>
#include <iostream>
#include <map>
#include <memory>
#include <string>

#include "ba_plan.hpp"

using namespace visfs_ba;
typedef std::vector<long long> Vals;

static std::map<std::string, Vals> in;
static long long scalar(const char* name, long long dflt = 0) { auto it = in.find(name); return it == in.end() || it->second.empty() ? dflt : it->second[0]; }
template <typename T> static std::vector<T> array_of(const char* name) { const Vals& v = in[name]; return std::vector<T>(v.begin(), v.end()); }

// the answers of the kernel-side predicates, as the test gives them (the driver has no kernels to ask)
static long long band_ok, band_rows_answer, band_lds_answer, cu_fits;
static size_t stub_band_lds_bytes(int npf, int B, int rows) { return (size_t)(100000 * npf + 1000 * B + rows); }
static bool stub_band_plan(int npf, int, int* rows, int* lds) { *rows = band_rows_answer ? (int)band_rows_answer : npf; *lds = (int)band_lds_answer; return band_ok != 0; }
static bool stub_pcg_cu_fits(int, int) { return cu_fits != 0; }

template <typename V> static void put(const char* name, const V& v, size_t n) { std::printf("%s %zu", name, n); for (size_t i = 0; i < n; ++i) std::printf(" %lld", (long long)v[i]); std::printf("\n"); }
template <typename V> static void put(const char* name, const V& v) { put(name, v, v.size()); }
static void put1(const char* name, long long v) { std::printf("%s 1 %lld\n", name, v); }
static void put_desc(const char* name, const std::vector<Desc4>& d, size_t n) {
    std::printf("%s %zu", name, 4 * n);
    for (size_t i = 0; i < n; ++i) std::printf(" %d %d %d %d", d[i].x, d[i].y, d[i].z, d[i].w);
    std::printf("\n");
}

int main() {
    std::string name; size_t n;
    while (std::cin >> name >> n) { Vals v(n); for (auto& x : v) std::cin >> x; in[name] = v; }
    const std::vector<uint8_t> pose_fixed = array_of<uint8_t>("pose_fixed"), point_fixed = array_of<uint8_t>("point_fixed");
    const std::vector<int32_t> obs_pose = array_of<int32_t>("obs_pose"), obs_point = array_of<int32_t>("obs_point");
    const std::vector<int32_t> odo_from = array_of<int32_t>("odo_from"), odo_to = array_of<int32_t>("odo_to");
    visfs_ba_graph gr{};
    gr.n_poses = (int)pose_fixed.size(); gr.n_points = (int)point_fixed.size(); gr.n_obs = (int)obs_pose.size(); gr.n_odo = (int)odo_from.size();
    gr.pose_fixed = pose_fixed.data(); gr.point_fixed = point_fixed.data(); gr.obs_pose = obs_pose.data(); gr.obs_point = obs_point.data();
    gr.odo_from = odo_from.data(); gr.odo_to = odo_to.data();
    gr.n_laser = (int)scalar("n_laser"); gr.laser_pose = (int)scalar("laser_pose");

    PlanDecisions D;
    D.solver = (int)scalar("solver"); D.batch_member = scalar("batch_member") != 0; D.throughput = scalar("throughput") != 0;
    D.index_blocks = (int)scalar("index_blocks", 1);
    D.sw.schur_runs = scalar("schur_runs") != 0; D.sw.run_lr = (int)scalar("run_lr"); D.sw.run_m = (int)scalar("run_m");
    D.sw.sch_passes = (int)scalar("sch_passes"); D.sw.pcg1 = scalar("pcg1", 1) != 0; D.sw.pcg_cu = (int)scalar("pcg_cu", -1);
    D.sw.band = scalar("band", 1) != 0; D.sw.band_rows = (int)scalar("band_rows"); D.sw.group = (int)scalar("group");
    band_ok = scalar("band_plan_ok", 1); band_rows_answer = scalar("band_plan_rows"); band_lds_answer = scalar("band_plan_lds", 4096); cu_fits = scalar("pcg_cu_fits", 1);
    D.band_plan = stub_band_plan; D.band_lds_bytes = stub_band_lds_bytes; D.pcg_cu_fits = stub_pcg_cu_fits;

    UploadPlan P;
    plan_poses(P, gr.pose_fixed, gr.n_poses);
    PlanGraph G;
    G.Np = gr.n_poses; G.Nl = gr.n_points; G.No = gr.n_obs; G.Ne = gr.n_odo; G.odo_from = gr.odo_from; G.odo_to = gr.odo_to; G.laser_pose = gr.laser_pose;
    G.Nz = (gr.n_laser > 0 && !pose_fixed[gr.laser_pose]) ? gr.n_laser : 0;          // (ws_upload: laser edges are active only while their pose is free)

    const int threads = (int)scalar("threads", 1);
    std::unique_ptr<WorkerPool> pool;
    if (threads > 1) pool.reset(new WorkerPool(threads - 1));
    GraphSummary sum;
    std::vector<SummaryPart> part; std::vector<int32_t> run;
    summarize_graph(&gr, P.pose_free.data(), P.Npf, pool.get(), true, sum, part, run);
    if (sum.bad) { std::printf("bad_graph 0\nmsg %s\n", sum.bad); return 0; }
    if (scalar("pairs_seen", -1) >= 0) sum.pairs_seen = scalar("pairs_seen");         // synthetic: the refusal of a pair list beyond 2^31 - 1
    put("cnt", sum.cnt); put("pcount", sum.pcount); put1("pairs_seen", sum.pairs_seen); put1("n_edges_ok", sum.n_edges_ok);
    { std::vector<int32_t> g; for (const RunGroup& q : sum.grp) { g.push_back(q.cnt); g.push_back(q.lo); g.push_back(q.hi); } put("grp", g); }

    const bool ok = plan_upload(P, G, sum, D);
    put1("status", P.status);
    if (!ok) { std::printf("msg %s\n", P.msg); return 0; }
    put("pose_free", P.pose_free); put("free_pose", P.free_pose);
    put("chunk_pose", P.chunk_pose); put("chunk_ptr", P.chunk_ptr); put("pose_chunk_ptr", P.pose_chunk_ptr);
    put("pose_odo_ptr", P.pose_odo_ptr); put("pose_odo", P.pose_odo);
    put("blk_i", P.blk_i); put("blk_j", P.blk_j); put("blk_ptr", P.blk_ptr); put("blk_of", P.blk_of);
    put("blk_odo_ptr", P.blk_odo_ptr); put("blk_odo", P.blk_odo);
    put("row_ptr", P.row_ptr); put("row_col", P.row_col); put("row_blk", P.row_blk);
    put("blk_chunk_ptr", P.blk_chunk_ptr); put("sch_blk", P.sch_blk);
    put_desc("sch_desc", P.sch_desc, P.n_sch); put_desc("blk_desc", P.blk_desc, 2 * (size_t)P.n_blk);
    put("fin_exp", P.fin_exp); put("diag_blk", P.diag_blk);
    put("pcg1_code", P.pcg1_code); put("blk_slot", P.blk_slot, P.n_blk); put("band_code", P.band_code);
    put1("sizeof_sch_desc", (long long)P.sch_desc.size()); put1("sizeof_blk_desc", (long long)P.blk_desc.size()); put1("sizeof_blk_slot", (long long)P.blk_slot.size());
    put1("run_LR", P.run.LR); put1("run_M", P.run.M); put1("run_n", P.run.n); put1("run_cap", P.run.cap); put1("run_wmax", P.run.wmax);
    put1("run_lds", (long long)P.run.lds); put1("run_total", P.run.total);
    put_desc("run_desc", P.run.desc, P.run.desc.size()); put("run_first", P.run.first); put("run_last", P.run.last); put("run_k0", P.run.k0);
    put1("Npf", P.Npf); put1("n_pose_obs", P.n_pose_obs); put1("n_chunks", P.n_chunks); put1("n_blk", P.n_blk); put1("n_sch", P.n_sch); put1("npairs", P.npairs);
    put1("sch_chunk", P.sch_chunk); put1("max_row", P.max_row); put1("pcg_rpw", P.pcg_rpw); put1("pcg_lds", (long long)P.pcg_lds); put1("lds_srow", P.lds_srow);
    put1("cu_T", P.cu_T); put1("cu_max_row", P.cu_max_row); put1("pcg1", P.pcg1); put1("pcg_cu", P.pcg_cu); put1("small_fits", P.small_fits);
    put1("band_B", P.band_B); put1("band_rows", P.band_rows); put1("band_lds", P.band_lds);
    put1("group", P.group); put1("n_lin_a", P.n_lin_a); put1("n_parts", P.n_parts); put1("chol_np", (long long)P.chol_np); put1("n_hist", (long long)P.n_hist);
    return 0;
}
