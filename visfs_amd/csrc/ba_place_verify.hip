// A place query whose candidates are verified by PnP in the same call (include/visfs_place_verify.h), two ways
// over the arithmetic of ba_place.hpp, ba_pnp.hpp and ba_place_verify.hpp:
//   * the one-core twin (a verifier on a store made on NULL): visfs_place_query, one visfs_pnp_solve per candidate on a host solver,
//     guided_twin and pnp::host_refine_from in sequence;
//   * device, on the stream of the store's handle, behind k_place_match and k_place_rank (place::launch_query), whose result block
//     heads the arena of this call:
//       k_place_verify_rows   grid z = 8, one workgroup of 512 per candidate: thread t takes row[c][t]; the rows with a finite point
//                             are compacted by ballot prefix into the candidate's pnp::Row list and match index, with m, the zeroed
//                             winner key and the result of a stage that does not run.  n_candidates is read on the device.
//       k_pnp_ransac_g, k_pnp_refine_g   pnp::group_pnp with n = 8 on those lists (stage 1)
//       k_place_guided        one workgroup of 512 per candidate: the queries' pixels, descriptors and valid flags staged in LDS;
//                             thread t owns entry t (eight words in registers), projects it with the stage-1 model and walks the
//                             queries, the Hamming distance only inside the window; after a barrier thread t owns query t and
//                             walks the picks; the kept pairs are compacted by ballot prefix in ascending query order into the
//                             result block and the stage-2 row list.  No atomic: every value is a minimum of integers.
//       k_pnp_refine_from_g   pnp::group_refine_from with n = 8: the refinement loop from the stage-1 model (stage 2)
// One upload (the parameters and the sixteen records), seven launches, one download (the arena), one wait.  The transform and the
// covariance are finished on the host by pnp::finalize in both flavours, so query_xyz never goes up.
#include "ba_place_verify.hpp"
#include "ba_pnp.hpp"
#include "ba_place_object.hpp"
#include "ba_group.hpp"
#include "ba_host.hpp"
#include "../../include/visfs_place_verify.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

using namespace host;

namespace place_verify {

constexpr int kC = place::kMaxCandidates, kP = place::kMaxPoints, kT = 512;
static_assert(kT == kP, "a thread per row, per entry and per query");

struct DevParams {                         // what the kernels of this file read of a call
    int32_t guided, max_distance, min_inliers, pad;
    double r2;
    pnp::Cam K;
};

struct CandRaw {                           // what the device leaves of a candidate; every word is written in every call
    int32_t m1, ran2, m2, pad;
    pnp::Result res1, res2;
    int32_t match1[kP], inl1[kP], inl2[kP];
    visfs_place_row row2[kP];
};
static_assert(sizeof(CandRaw) % 8 == 0 && sizeof(pnp::Result) % 8 == 0 && sizeof(visfs_place_result) % 8 == 0, "doubles stay aligned in the arena");

struct Arena {                             // one download
    visfs_place_result place;
    CandRaw cand[kC];
};

struct UpBlock {                           // one upload
    place::Params q;
    int32_t pad;
    DevParams p;
    pnp::PnpRec rec1[kC];
    pnp::RefineFromRec rec2[kC];
};

struct Bufs {                              // by value to the kernels of this file
    Arena* arena;
    pnp::Row* rows1;                       // [8][512]
    pnp::Row* rows2;
    unsigned long long* keys;              // [8]
    int32_t* pick;                         // [8][512]
    int32_t* keep;
};

// an entry's pixel under the stage-1 model, or false: a point that is not finite, a depth that is not positive, a pixel that is not finite
BA_HD bool project_entry(const visfs_ba::Rt& T, const pnp::Cam& K, const float* xyz, double& pu, double& pv) {
    const pnp::Row r{ xyz[0], xyz[1], xyz[2], 0.0f, 0.0f };
    if (!(r.X - r.X == 0.0f) || !(r.Y - r.Y == 0.0f) || !(r.Z - r.Z == 0.0f)) return false;
    const visfs_ba::Vec3 pc = visfs_ba::mat_vec(T.R, visfs_ba::Vec3{ (double)r.X, (double)r.Y, (double)r.Z });
    const double z = pc.z + T.t.z;
    if (!(z > 0.0)) return false;
    pnp::project(T, K, r, pu, pv);
    return pu - pu == 0.0 && pv - pv == 0.0;
}

// the position of a flagged thread among the flagged of its workgroup, and their number; every thread of the workgroup calls it
__device__ __forceinline__ int wg_prefix(bool flag, int32_t* wcount, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wcount[wave] = (int32_t)__popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < kT / 64; ++q) {
        if (q < wave) before += wcount[q];
        total += wcount[q];
    }
    __syncthreads();
    return before + (int)__popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kT) void k_place_verify_rows(Bufs B) {
    const int c = blockIdx.z, t = threadIdx.x;
    __shared__ int32_t wcount[kT / 64];
    const visfs_place_result& R = B.arena->place;
    CandRaw& C = B.arena->cand[c];
    uint32_t* words = reinterpret_cast<uint32_t*>(&C);
    for (int q = t; q < (int)(sizeof(CandRaw) / 4); q += kT) words[q] = 0u;
    B.pick[c * kP + t] = kNone;
    B.keep[c * kP + t] = kNone;
    __syncthreads();
    const int nc = min(max(R.n_candidates, 0), kC);
    const int count = c < nc ? min(max(R.candidate[c].count, 0), kP) : 0;
    pnp::Row r{ 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
    if (t < count) {
        const visfs_place_row& w = R.row[c][t];
        r = pnp::Row{ w.from_xyz[0], w.from_xyz[1], w.from_xyz[2], w.to_xy[0], w.to_xy[1] };
    }
    const bool enters = t < count && r.X - r.X == 0.0f && r.Y - r.Y == 0.0f && r.Z - r.Z == 0.0f;
    int m;
    const int o = wg_prefix(enters, wcount, m);
    if (enters) { B.rows1[c * kP + o] = r; C.match1[o] = t; }
    if (t == 0) {
        C.m1 = m;
        B.keys[c] = 0ull;                                              // no winner yet
        C.res1.winner = -1;                                            // (the rest of the two results is zero already)
        C.res2.winner = -1;
    }
}

__global__ __launch_bounds__(kT) void k_place_guided(Bufs B, const DevParams* __restrict__ prm, const place::SetBlock* __restrict__ set, int nq,
                                                     const place::SlotBlock* __restrict__ slots, const place::Payload* __restrict__ pay) {
    const int c = blockIdx.z, t = threadIdx.x;
    __shared__ uint32_t s_desc[kP * kDescWords];
    __shared__ float s_xy[kP * 2];
    __shared__ uint8_t s_valid[kP];
    __shared__ int32_t s_pick[kP];
    __shared__ int32_t wcount[kT / 64];
    const DevParams P = *prm;
    const visfs_place_result& R = B.arena->place;
    CandRaw& C = B.arena->cand[c];
    const int nc = min(max(R.n_candidates, 0), kC);
    if (c >= nc || !P.guided || C.res1.n_inliers < P.min_inliers) return;           // the same for every thread of the workgroup
    const int slot = R.candidate[c].slot;
    const place::SlotBlock& S = slots[slot];
    const place::Payload& Y = pay[slot];
    const int ne = min(max(Y.n, 0), kP);
    nq = min(max(nq, 0), kP);
    for (int q = t; q < nq * kDescWords; q += kT) s_desc[q] = (&set->desc[0][0])[q];
    for (int q = t; q < nq * 2; q += kT) s_xy[q] = (&set->xy[0][0])[q];
    s_valid[t] = t < nq ? set->valid[t] : (uint8_t)0;
    __syncthreads();
    // thread t owns entry t
    int32_t pick = kNone;
    if (t < ne && S.valid[t]) {
        double tq[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) tq[i] = C.res1.tq[i];
        const visfs_ba::Rt T = pnp::tq_to_rt(tq);
        double pu, pv;
        if (project_entry(T, P.K, Y.xyz[t], pu, pv)) {
            uint32_t e[kDescWords];
#pragma unroll
            for (int q = 0; q < kDescWords; ++q) e[q] = S.desc[t][q];
            pick = pick_of(e, pu, pv, s_desc, s_valid, s_xy, nq, P.r2, P.max_distance);
        }
    }
    s_pick[t] = pick;
    B.pick[c * kP + t] = pick;
    __syncthreads();
    // thread t owns query t
    const int32_t keep = t < nq ? keep_of(t, s_pick, ne) : kNone;
    B.keep[c * kP + t] = keep;
    int m2;
    const int o = wg_prefix(keep != kNone, wcount, m2);
    if (keep != kNone) {
        const int j = keep & 1023;
        visfs_place_row& w = C.row2[o];
        w.query_index = t; w.db_index = j; w.distance = keep >> 10; w.id = Y.id[j];
        w.from_xyz[0] = Y.xyz[j][0]; w.from_xyz[1] = Y.xyz[j][1]; w.from_xyz[2] = Y.xyz[j][2];
        w.to_xy[0] = s_xy[2 * t]; w.to_xy[1] = s_xy[2 * t + 1];
        B.rows2[c * kP + o] = pnp::Row{ w.from_xyz[0], w.from_xyz[1], w.from_xyz[2], w.to_xy[0], w.to_xy[1] };
    }
    if (t == 0) { C.ran2 = 1; C.m2 = m2; }
}

}  // namespace place_verify

using namespace place_verify;

// ---------------------------------------------------------------- the object
struct visfs_place_verifier {
    std::string err;
    visfs_place_db* db = nullptr;
    bool device = false;
    bool called = false;
    place::Counts4 counts;
    pnp::PnpShape shape{};                 // of the last call
    int32_t n_cand = 0;
    int32_t m1[kC] = {}, m2[kC] = {}, ran2[kC] = {};
    pnp::Result res1[kC] = {}, res2[kC] = {};

    // host scratch of a call, sized at creation: a candidate's rows as arrays and as pnp::Row, the gathered to_xyz, the identity match
    // index of the guided rows, an inlier list, and the twin's projections
    std::vector<float> s_from, s_to, s_xyz;
    std::vector<pnp::Row> s_rows;
    std::vector<int32_t> s_list, s_identity;
    std::vector<double> s_pu, s_pv;
    std::vector<uint8_t> s_ok;

    // the twin
    visfs_pnp* solver1[kC] = {};
    visfs_pnp* solver2[kC] = {};
    std::vector<int32_t> h_pick, h_keep;   // [8][512]

    // device
    int dev = 0;
    hipStream_t stream = nullptr;
    PinnedBuf<UpBlock> h_up;               // pinned
    DeviceBuf<UpBlock> d_up;
    PinnedBuf<Arena> h_arena;              // pinned
    DeviceBuf<char> d_state;               // the arena, the row lists, the keys, the hypotheses and the passes of both stages
    Bufs B{};
    pnp::PnpRec rec1[kC] = {};             // device addresses; K is the call's
    pnp::RefineFromRec rec2[kC] = {};

    ~visfs_place_verifier() {              // before the members free what they own
        for (int c = 0; c < kC; ++c) {
            if (solver1[c]) visfs_pnp_destroy(solver1[c]);
            if (solver2[c]) visfs_pnp_destroy(solver2[c]);
        }
        if (!device) return;
        (void)hipSetDevice(dev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

struct Carver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t n) {
        T* p = reinterpret_cast<T*>(base + off);
        off += up256(sizeof(T) * n);
        return p;
    }
};

// the same carve twice: on a null base for the size, on the allocation for the addresses
size_t carve(visfs_place_verifier* v, char* base) {
    Carver k{ base };
    const size_t H = pnp::kMaxHypotheses, Rf = pnp::kMaxRefine;
    v->B.arena = k.take<Arena>(1);
    v->B.rows1 = k.take<pnp::Row>((size_t)kC * kP);
    v->B.rows2 = k.take<pnp::Row>((size_t)kC * kP);
    v->B.keys = k.take<unsigned long long>(kC);
    v->B.pick = k.take<int32_t>((size_t)kC * kP);
    v->B.keep = k.take<int32_t>((size_t)kC * kP);
    for (int c = 0; c < kC; ++c) {
        CandRaw* C = &v->B.arena->cand[c];
        pnp::PnpRec& a = v->rec1[c];
        a.m = &C->m1; a.rows = v->B.rows1 + (size_t)c * kP; a.key = v->B.keys + c;
        a.samples = k.take<int32_t>(4 * H); a.vc = k.take<int32_t>(2 * H); a.models = k.take<double>(12 * H);
        a.res = &C->res1; a.inliers = C->inl1;
        a.pass_tq = k.take<double>(7 * Rf); a.pass_thr = k.take<float>(Rf); a.pass_cnt = k.take<int32_t>(Rf);
        a.pass_lists = k.take<int32_t>(Rf * kP);
        a.cap = kP; a.skip = 0;
        pnp::RefineFromRec& b = v->rec2[c];
        b.m = &C->m2; b.rows = v->B.rows2 + (size_t)c * kP; b.ran = &C->ran2; b.start = &C->res1;
        b.res = &C->res2; b.inliers = C->inl2;
        b.pass_tq = k.take<double>(7 * Rf); b.pass_thr = k.take<float>(Rf); b.pass_cnt = k.take<int32_t>(Rf);
        b.pass_lists = k.take<int32_t>(Rf * kP);
        b.cap = kP; b.pad = 0;
    }
    return k.off;
}

int device_init(visfs_place_verifier* v) {
    HIP_TRY(v, hipSetDevice(v->dev));
    const size_t bytes = carve(v, nullptr);
    RC_TRY(v->d_state.alloc(v, bytes));
    RC_TRY(v->d_up.alloc(v, 1));
    RC_TRY(v->h_up.alloc(v, 1));
    RC_TRY(v->h_arena.alloc(v, 1));
    HIP_TRY(v, hipMemsetAsync(v->d_state.get(), 0, bytes, v->stream));
    HIP_TRY(v, hipStreamSynchronize(v->stream));
    (void)carve(v, v->d_state.get());
    return VISFS_BA_OK;
}

int check_verify(const visfs_place_verify_params& p, const char** why) {
    const int rc = pnp::check_params(p.pnp, p.camera, why);
    if (rc != VISFS_BA_OK) return rc;
    if (!std::isfinite(p.guided_radius) || p.guided_radius < 0.0f) { *why = "guided_radius is not finite or is negative"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    if (p.guided_max_distance < 0 || p.guided_max_distance > 256) { *why = "guided_max_distance must lie in 0 .. 256"; return VISFS_BA_ERR_BAD_ARGUMENT; }
    return VISFS_BA_OK;
}

// What visfs_pnp_solve does behind its search, for a stage whose model and inlier list (numbers of `rows`) are known: the sentinel
// with the identity covariance, or pnp::finalize.  matches[k]: the input row of rows[k]; to_xyz per input row, or NULL.
void finish_stage(const pnp::Result& res, const pnp::Row* rows, const int32_t* list, const int32_t* matches, const float* to_xyz,
                  const visfs_place_verify_params& p, int min_inliers, double* T, double* cov, int32_t* inliers_out, int32_t* n_inliers) {
    for (int i = 0; i < 16; ++i) T[i] = 0.0;
    for (int i = 0; i < 36; ++i) cov[i] = (i % 7 == 0) ? 1.0 : 0.0;
    *n_inliers = 0;
    if (res.n_inliers < min_inliers) return;
    const pnp::Cam K{ p.camera.fx, p.camera.fy, p.camera.cx, p.camera.cy };
    pnp::finalize(res, rows, p.camera.Tir, K, list, (size_t)res.n_inliers, matches, to_xyz, T, cov);
    *n_inliers = res.n_inliers;
    for (int32_t i = 0; i < res.n_inliers; ++i) inliers_out[i] = matches[list[i]];
}

// to_xyz of visfs_pnp_solve for rows[0 .. n): query_xyz at the rows' query_index
const float* gather_xyz(const float* query_xyz, const visfs_place_row* rows, int n, std::vector<float>& out) {
    if (!query_xyz) return nullptr;                                     // (out holds 3 x 512 floats since the verifier was made)
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) out[3 * (size_t)i + k] = query_xyz[3 * (size_t)rows[i].query_index + k];
    return out.data();
}

void pick_best(visfs_place_verify_result* V, int n_cand, int min_inliers) {
    V->best = -1;
    int32_t most = -1;
    for (int c = 0; c < n_cand; ++c) {
        const visfs_place_verify_candidate& k = V->candidate[c];
        const int32_t n = k.stage2.ran ? k.stage2.n_inliers : k.stage1.n_inliers;
        if (n >= min_inliers && n > most) { most = n; V->best = c; }
    }
}

int host_call(visfs_place_verifier* v, const visfs_place_set* s, const visfs_place_params& pp, const visfs_place_verify_params& vp,
              const float* query_xyz, visfs_place_result* R, visfs_place_verify_result* V) {
    visfs_place_db* db = v->db;
    const place::Counts4 before = db->counts;
    const int rc = visfs_place_query(db, s, &pp, R);
    db->counts = before;                                               // last_counts of the store reports its own queries
    if (rc != VISFS_BA_OK) return fail(v, rc, db->err);
    const int min_inliers = v->shape.min_inliers;
    const pnp::Cam K{ vp.camera.fx, vp.camera.fy, vp.camera.cx, vp.camera.cy };
    std::fill(v->h_pick.begin(), v->h_pick.end(), kNone);
    std::fill(v->h_keep.begin(), v->h_keep.end(), kNone);
    v->n_cand = R->n_candidates;
    std::vector<float>&from = v->s_from, &to = v->s_to, &xyz = v->s_xyz;
    std::vector<pnp::Row>& rows2 = v->s_rows;
    std::vector<int32_t>&list = v->s_list, &identity = v->s_identity;
    std::vector<double>&pu = v->s_pu, &pv = v->s_pv;
    std::vector<uint8_t>& ok = v->s_ok;
    const place::SetBlock& Q = *s->host;
    for (int c = 0; c < kC; ++c) { v->m1[c] = v->m2[c] = v->ran2[c] = 0; v->res1[c] = v->res2[c] = pnp::Result{}; v->res1[c].winner = v->res2[c].winner = -1; }
    for (int c = 0; c < R->n_candidates; ++c) {
        visfs_place_verify_candidate& k = V->candidate[c];
        const int count = R->candidate[c].count;
        const visfs_place_row* rows = R->row[c];
        for (int i = 0; i < count; ++i) {
            std::memcpy(&from[3 * (size_t)i], rows[i].from_xyz, 12);
            std::memcpy(&to[2 * (size_t)i], rows[i].to_xy, 8);
        }
        const int rc1 = visfs_pnp_solve(v->solver1[c], &vp.pnp, &vp.camera, count, from.data(), to.data(), gather_xyz(query_xyz, rows, count, xyz),
                                        k.stage1.T, k.stage1.cov, k.stage1.matches, &k.stage1.n_matches, k.stage1.inliers, &k.stage1.n_inliers);
        if (rc1 != VISFS_BA_OK) return fail(v, rc1, std::string("stage 1: ") + visfs_pnp_last_error(v->solver1[c]));
        v->m1[c] = k.stage1.n_matches;
        v->res1[c] = pnp::last_result(v->solver1[c]);
        if (!vp.guided || k.stage1.n_inliers < min_inliers) continue;
        // stage 2
        const int slot = R->candidate[c].slot;
        const place::SlotBlock& S = db->hslots[(size_t)slot];
        const place::Payload& Y = db->hpay[(size_t)slot];
        const visfs_ba::Rt T = pnp::tq_to_rt(v->res1[c].tq);
        for (int j = 0; j < Y.n; ++j) ok[(size_t)j] = S.valid[j] && project_entry(T, K, Y.xyz[j], pu[(size_t)j], pv[(size_t)j]);
        int32_t* pick = v->h_pick.data() + (size_t)c * kP;
        int32_t* keep = v->h_keep.data() + (size_t)c * kP;
        const int m2 = guided_twin(pu.data(), pv.data(), ok.data(), &S.desc[0][0], Y.n, &Q.desc[0][0], Q.valid, &Q.xy[0][0], s->n,
                                   radius2(vp.guided_radius), vp.guided_max_distance, pick, keep);
        int o = 0;
        for (int i = 0; i < s->n; ++i) {
            if (keep[i] == kNone) continue;
            const int j = keep[i] & 1023;
            visfs_place_row& w = k.stage2.row[o];
            w.query_index = i; w.db_index = j; w.distance = keep[i] >> 10; w.id = Y.id[j];
            std::memcpy(w.from_xyz, Y.xyz[j], 12);
            std::memcpy(w.to_xy, Q.xy[i], 8);
            rows2[(size_t)o] = pnp::Row{ w.from_xyz[0], w.from_xyz[1], w.from_xyz[2], w.to_xy[0], w.to_xy[1] };
            ++o;
        }
        k.stage2.ran = 1; k.stage2.n_rows = m2;
        v->ran2[c] = 1; v->m2[c] = m2;
        const int rc2 = pnp::host_refine_from(v->solver2[c], rows2.data(), m2, K, v->shape, v->res1[c].tq, &v->res2[c], &list);
        if (rc2 != VISFS_BA_OK) return fail(v, rc2, "stage 2: the host refinement refused its rows");
        finish_stage(v->res2[c], rows2.data(), list.data(), identity.data(), gather_xyz(query_xyz, k.stage2.row, m2, xyz), vp, min_inliers,
                     k.stage2.T, k.stage2.cov, k.stage2.inliers, &k.stage2.n_inliers);
    }
    pick_best(V, R->n_candidates, min_inliers);
    v->counts = place::Counts4{};
    return VISFS_BA_OK;
}

int device_call(visfs_place_verifier* v, const visfs_place_set* s, const place::Params& q, const visfs_place_verify_params& vp,
                const float* query_xyz, visfs_place_result* R, visfs_place_verify_result* V) {
    visfs_place_db* db = v->db;
    HIP_TRY(v, hipSetDevice(v->dev));
    const pnp::Cam K{ vp.camera.fx, vp.camera.fy, vp.camera.cx, vp.camera.cy };
    const int min_inliers = v->shape.min_inliers;
    // (every call ends in a wait behind its download, so the pinned blocks are free)
    UpBlock& U = *v->h_up.get();
    U.q = q; U.pad = 0;
    U.p = DevParams{ vp.guided ? 1 : 0, vp.guided_max_distance, min_inliers, 0, radius2(vp.guided_radius), K };
    for (int c = 0; c < kC; ++c) {
        U.rec1[c] = v->rec1[c]; U.rec1[c].K = K;
        U.rec2[c] = v->rec2[c]; U.rec2[c].K = K;
    }
    place::Counts4 n;
    HIP_TRY(v, hipMemcpyAsync(v->d_up.get(), v->h_up.get(), sizeof(UpBlock), hipMemcpyHostToDevice, v->stream));
    ++n.uploads;
    const int launched = place::launch_query(db, s, q, &v->d_up->q, &v->B.arena->place);
    if (launched < 0) { HIP_TRY(v, hipGetLastError()); return fail(v, VISFS_BA_ERR_DEVICE, "a launch of the query was refused"); }
    n.launches += launched;
    hipLaunchKernelGGL(k_place_verify_rows, dim3(1, 1, kC), dim3(kT), 0, v->stream, v->B);
    HIP_TRY(v, hipGetLastError());
    ++n.launches;
    flow::GroupCounts g{};
    if (pnp::group_pnp(v->stream, kC, v->d_up->rec1, v->shape, &g) != VISFS_BA_OK) return fail(v, VISFS_BA_ERR_DEVICE, "a launch of stage 1 was refused");
    hipLaunchKernelGGL(k_place_guided, dim3(1, 1, kC), dim3(kT), 0, v->stream, v->B, &v->d_up->p, s->d_set.get(), s->n, db->d_slots.get(), db->d_pay.get());
    HIP_TRY(v, hipGetLastError());
    ++n.launches;
    if (pnp::group_refine_from(v->stream, kC, v->d_up->rec2, v->shape, &g) != VISFS_BA_OK) return fail(v, VISFS_BA_ERR_DEVICE, "the launch of stage 2 was refused");
    n.launches += g.launches;
    HIP_TRY(v, hipMemcpyAsync(v->h_arena.get(), v->B.arena, sizeof(Arena), hipMemcpyDeviceToHost, v->stream));
    ++n.downloads;
    HIP_TRY(v, hipStreamSynchronize(v->stream));
    ++n.waits;
    const Arena& A = *v->h_arena.get();
    if (A.place.n_slots != q.n_slots || A.place.n_candidates < 0 || A.place.n_candidates > kC)
        return fail(v, VISFS_BA_ERR_DEVICE, "the ranking returned an impossible block");
    std::memcpy(R, &A.place, sizeof(*R));
    std::vector<pnp::Row>& rows = v->s_rows;
    std::vector<int32_t>& identity = v->s_identity;
    std::vector<float>& xyz = v->s_xyz;
    v->n_cand = R->n_candidates;
    for (int c = 0; c < kC; ++c) {
        const CandRaw& C = A.cand[c];
        v->m1[c] = C.m1; v->m2[c] = C.m2; v->ran2[c] = C.ran2; v->res1[c] = C.res1; v->res2[c] = C.res2;
    }
    for (int c = 0; c < R->n_candidates; ++c) {
        const CandRaw& C = A.cand[c];
        visfs_place_verify_candidate& k = V->candidate[c];
        const int count = R->candidate[c].count;
        bool sane = count >= 0 && count <= kP && C.m1 >= 0 && C.m1 <= count && C.m2 >= 0 && C.m2 <= kP && C.res1.n_inliers >= 0 &&
                    C.res1.n_inliers <= C.m1 && C.res2.n_inliers >= 0 && C.res2.n_inliers <= C.m2 && C.res1.n_passes >= 0 &&
                    C.res1.n_passes <= pnp::kMaxRefine && C.res2.n_passes >= 0 && C.res2.n_passes <= pnp::kMaxRefine;
        for (int i = 0; sane && i < C.m1; ++i) sane = C.match1[i] >= 0 && C.match1[i] < count;
        for (int i = 0; sane && i < C.res1.n_inliers; ++i) sane = C.inl1[i] >= 0 && C.inl1[i] < C.m1;
        for (int i = 0; sane && i < C.res2.n_inliers; ++i) sane = C.inl2[i] >= 0 && C.inl2[i] < C.m2;
        for (int i = 0; sane && i < C.m2; ++i) sane = C.row2[i].query_index >= 0 && C.row2[i].query_index < kP;
        if (!sane) return fail(v, VISFS_BA_ERR_DEVICE, "the verification returned an impossible count or row number");
        const visfs_place_row* in = R->row[c];
        for (int i = 0; i < C.m1; ++i) {
            const visfs_place_row& w = in[C.match1[i]];
            rows[(size_t)i] = pnp::Row{ w.from_xyz[0], w.from_xyz[1], w.from_xyz[2], w.to_xy[0], w.to_xy[1] };
        }
        k.stage1.n_matches = C.m1;
        std::copy(C.match1, C.match1 + C.m1, k.stage1.matches);
        finish_stage(C.res1, rows.data(), C.inl1, C.match1, gather_xyz(query_xyz, in, count, xyz), vp, min_inliers, k.stage1.T, k.stage1.cov,
                     k.stage1.inliers, &k.stage1.n_inliers);
        if (!C.ran2) continue;
        k.stage2.ran = 1; k.stage2.n_rows = C.m2;
        std::copy(C.row2, C.row2 + C.m2, k.stage2.row);
        for (int i = 0; i < C.m2; ++i) {
            const visfs_place_row& w = C.row2[i];
            rows[(size_t)i] = pnp::Row{ w.from_xyz[0], w.from_xyz[1], w.from_xyz[2], w.to_xy[0], w.to_xy[1] };
        }
        finish_stage(C.res2, rows.data(), C.inl2, identity.data(), gather_xyz(query_xyz, C.row2, C.m2, xyz), vp, min_inliers, k.stage2.T,
                     k.stage2.cov, k.stage2.inliers, &k.stage2.n_inliers);
    }
    pick_best(V, R->n_candidates, min_inliers);
    v->counts = n;
    return VISFS_BA_OK;
}

bool finite_all(const double* a, int n) {
    for (int i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
    return true;
}

}  // namespace

// ====================================================================== exported C ABI
extern "C" {

int visfs_place_verify_abi_version(void) { return VISFS_PLACE_VERIFY_ABI_VERSION; }

void visfs_place_verify_default_params(visfs_place_verify_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    visfs_pnp_default_params(&p->pnp);
    p->guided = 1;
    p->guided_radius = 3.0f * p->pnp.reproj_error;
    p->guided_max_distance = 64;
}

int visfs_place_verifier_create(visfs_place_db* db, visfs_place_verifier** out) {
    if (!db || !out) return VISFS_BA_ERR_BAD_ARGUMENT;
    *out = nullptr;
    return guarded(db, [&]() -> int {
        visfs_place_verifier* v = new visfs_place_verifier();
        v->db = db; v->device = db->device; v->dev = db->dev; v->stream = db->stream;
        v->s_from.assign((size_t)3 * kP, 0.0f); v->s_to.assign((size_t)2 * kP, 0.0f); v->s_xyz.assign((size_t)3 * kP, 0.0f);
        v->s_rows.assign((size_t)kP, pnp::Row{}); v->s_list.reserve((size_t)kP); v->s_identity.resize((size_t)kP);
        for (int i = 0; i < kP; ++i) v->s_identity[(size_t)i] = i;
        v->s_pu.assign((size_t)kP, 0.0); v->s_pv.assign((size_t)kP, 0.0); v->s_ok.assign((size_t)kP, 0);
        int rc = VISFS_BA_OK;
        if (v->device) {
            rc = device_init(v);
        } else {
            v->h_pick.assign((size_t)kC * kP, kNone); v->h_keep.assign((size_t)kC * kP, kNone);
            for (int c = 0; c < kC && rc == VISFS_BA_OK; ++c) {
                rc = visfs_pnp_create_host(kP, &v->solver1[c]);
                if (rc == VISFS_BA_OK) rc = visfs_pnp_create_host(kP, &v->solver2[c]);
            }
            if (rc != VISFS_BA_OK) v->err = "a host solver could not be made";
        }
        if (rc != VISFS_BA_OK) { db->err = v->err; delete v; return rc; }
        *out = v;
        return (int)VISFS_BA_OK;
    });
}

void visfs_place_verifier_destroy(visfs_place_verifier* v) { delete v; }

const char* visfs_place_verifier_last_error(const visfs_place_verifier* v) { return v ? v->err.c_str() : "null verifier"; }

int visfs_place_query_verify(visfs_place_verifier* v, const visfs_place_set* set, const visfs_place_params* place_params,
                             const visfs_place_verify_params* verify_params, const float* query_xyz, visfs_place_result* place_result,
                             visfs_place_verify_result* verify_result) {
    if (!v) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!set || !place_params || !verify_params || !place_result || !verify_result) return fail(v, VISFS_BA_ERR_BAD_ARGUMENT, "a required pointer is null");
    return guarded(v, [&]() -> int {
        const char* why = "";
        place::Params q;
        int rc = place::prepare_query(v->db, set, *place_params, &q, &why);
        if (rc == VISFS_BA_OK) rc = check_verify(*verify_params, &why);
        if (rc != VISFS_BA_OK) return fail(v, rc, why);
        const visfs_pnp_params& p = verify_params->pnp;
        v->shape = pnp::PnpShape{ p.iterations, p.min_inliers < 4 ? 4 : p.min_inliers, p.refine_iterations, p.reproj_error, p.refine_sigma, p.seed };
        v->called = false;
        std::memset(verify_result, 0, sizeof(*verify_result));
        verify_result->best = -1;
        rc = v->device ? device_call(v, set, q, *verify_params, query_xyz, place_result, verify_result)
                       : host_call(v, set, *place_params, *verify_params, query_xyz, place_result, verify_result);
        if (rc != VISFS_BA_OK) return rc;
        verify_result->status = VISFS_BA_OK;
        v->called = true;
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_verify_last_counts(const visfs_place_verifier* v, int32_t* uploads, int32_t* launches, int32_t* downloads, int32_t* waits) {
    if (!v) return VISFS_BA_ERR_BAD_ARGUMENT;
    return v->counts.read(uploads, launches, downloads, waits);
}

int visfs_place_verify_download_pnp(visfs_place_verifier* v, int32_t c, int32_t stage, int32_t* m, int32_t* n_hypotheses, int32_t* n_passes,
                                    int32_t* samples, int32_t* valid, double* models, int32_t* counts, int32_t* winner, double* refit_tq,
                                    double* pass_tq, float* pass_threshold, int32_t* pass_count, int32_t* pass_inliers) {
    if (!v) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(v, [&]() -> int {
        if (c < 0 || c >= kC || (stage != 1 && stage != 2)) return fail(v, VISFS_BA_ERR_BAD_ARGUMENT, "no such candidate or stage");
        if (!v->called) return fail(v, VISFS_BA_ERR_NOT_LOADED, "no call to report on");
        if (m) *m = 0;
        if (n_hypotheses) *n_hypotheses = 0;
        if (n_passes) *n_passes = 0;
        if (winner) *winner = -1;
        if (refit_tq) for (int i = 0; i < 7; ++i) refit_tq[i] = 0.0;
        if (c >= v->n_cand || (stage == 2 && !v->ran2[c])) return (int)VISFS_BA_OK;
        const pnp::Result& res = stage == 1 ? v->res1[c] : v->res2[c];
        const int32_t rows = stage == 1 ? v->m1[c] : v->m2[c];
        const size_t H = (stage == 1 && rows >= v->shape.min_inliers) ? (size_t)v->shape.iterations : 0, R = (size_t)res.n_passes;
        if (m) *m = rows;
        if (n_hypotheses) *n_hypotheses = (int32_t)H;
        if (n_passes) *n_passes = res.n_passes;
        if (winner) *winner = res.winner;
        if (refit_tq) for (int i = 0; i < 7; ++i) refit_tq[i] = res.refit0[i];
        if (!v->device) {
            visfs_pnp* s = stage == 1 ? v->solver1[c] : v->solver2[c];
            const int rc = visfs_pnp_download(s, samples, valid, models, counts, nullptr, nullptr, pass_tq, pass_threshold, pass_count, pass_inliers);
            if (rc != VISFS_BA_OK) return fail(v, rc, visfs_pnp_last_error(s));
            return (int)VISFS_BA_OK;
        }
        if (H == 0 && R == 0) return (int)VISFS_BA_OK;
        std::vector<int32_t> h_samples(4 * H), h_vc(2 * H), h_pcnt(pnp::kMaxRefine), h_plists(R * kP);
        std::vector<double> h_models(12 * H), h_ptq(7 * pnp::kMaxRefine);
        std::vector<float> h_pthr(pnp::kMaxRefine);
        HIP_TRY(v, hipSetDevice(v->dev));
        const pnp::PnpRec& a = v->rec1[c];
        const pnp::RefineFromRec& b = v->rec2[c];
        if (H > 0) {
            HIP_TRY(v, hipMemcpyAsync(h_samples.data(), a.samples, 16 * H, hipMemcpyDeviceToHost, v->stream));
            HIP_TRY(v, hipMemcpyAsync(h_vc.data(), a.vc, 8 * H, hipMemcpyDeviceToHost, v->stream));
            HIP_TRY(v, hipMemcpyAsync(h_models.data(), a.models, 96 * H, hipMemcpyDeviceToHost, v->stream));
        }
        if (R > 0) {
            HIP_TRY(v, hipMemcpyAsync(h_ptq.data(), stage == 1 ? a.pass_tq : b.pass_tq, 56 * R, hipMemcpyDeviceToHost, v->stream));
            HIP_TRY(v, hipMemcpyAsync(h_pthr.data(), stage == 1 ? a.pass_thr : b.pass_thr, 4 * R, hipMemcpyDeviceToHost, v->stream));
            HIP_TRY(v, hipMemcpyAsync(h_pcnt.data(), stage == 1 ? a.pass_cnt : b.pass_cnt, 4 * R, hipMemcpyDeviceToHost, v->stream));
            HIP_TRY(v, hipMemcpyAsync(h_plists.data(), stage == 1 ? a.pass_lists : b.pass_lists, 4 * R * kP, hipMemcpyDeviceToHost, v->stream));
        }
        HIP_TRY(v, hipStreamSynchronize(v->stream));
        for (size_t h = 0; h < H; ++h) {
            if (samples) for (int k = 0; k < 4; ++k) samples[4 * h + k] = h_samples[4 * h + k];
            if (valid) valid[h] = h_vc[2 * h];
            if (counts) counts[h] = h_vc[2 * h + 1];
            if (models) for (int k = 0; k < 12; ++k) models[12 * h + k] = h_models[12 * h + k];
        }
        for (size_t k = 0; k < R; ++k) {
            if (pass_tq) for (int i = 0; i < 7; ++i) pass_tq[7 * k + i] = h_ptq[7 * k + i];
            if (pass_threshold) pass_threshold[k] = h_pthr[k];
            if (pass_count) pass_count[k] = h_pcnt[k];
            const size_t cnt_k = (size_t)std::min(std::max(h_pcnt[k], 0), rows);
            if (pass_inliers)
                for (size_t i = 0; i < (size_t)rows; ++i) pass_inliers[k * (size_t)rows + i] = i < cnt_k ? h_plists[k * kP + i] : -1;
        }
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_verify_download_guided(visfs_place_verifier* v, int32_t c, int32_t* pick, int32_t* keep) {
    if (!v) return VISFS_BA_ERR_BAD_ARGUMENT;
    return guarded(v, [&]() -> int {
        if (c < 0 || c >= kC) return fail(v, VISFS_BA_ERR_BAD_ARGUMENT, "no such candidate");
        if (!v->called) return fail(v, VISFS_BA_ERR_NOT_LOADED, "no call to report on");
        if (!v->device) {
            if (pick) std::memcpy(pick, v->h_pick.data() + (size_t)c * kP, 4 * kP);
            if (keep) std::memcpy(keep, v->h_keep.data() + (size_t)c * kP, 4 * kP);
            return (int)VISFS_BA_OK;
        }
        HIP_TRY(v, hipSetDevice(v->dev));
        if (pick) HIP_TRY(v, hipMemcpyAsync(pick, v->B.pick + (size_t)c * kP, 4 * kP, hipMemcpyDeviceToHost, v->stream));
        if (keep) HIP_TRY(v, hipMemcpyAsync(keep, v->B.keep + (size_t)c * kP, 4 * kP, hipMemcpyDeviceToHost, v->stream));
        HIP_TRY(v, hipStreamSynchronize(v->stream));
        return (int)VISFS_BA_OK;
    });
}

int visfs_place_verify_hook_window(double pu, double pv, float qx, float qy, float radius) {
    return in_window(pu, pv, qx, qy, radius2(radius)) ? 1 : 0;
}

int visfs_place_closure_edge(const double T[16], const double cov[36], double z_out[3], double information_out[9], double out_of_plane[3]) {
    if (!T || !cov || !z_out || !information_out || !out_of_plane) return VISFS_BA_ERR_BAD_ARGUMENT;
    if (!finite_all(T, 16) || !finite_all(cov, 36)) return VISFS_BA_ERR_BAD_ARGUMENT;
    bool zero = true;
    for (int i = 0; i < 16; ++i) zero = zero && T[i] == 0.0;
    if (zero) return VISFS_BA_ERR_BAD_ARGUMENT;                        // the sentinel: no pose
    // the block over (x, y, yaw), symmetrised
    const int ix[3] = { 0, 1, 5 };
    double S[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) S[a][b] = 0.5 * (cov[6 * ix[a] + ix[b]] + cov[6 * ix[b] + ix[a]]);
    // Cholesky S = L L^T; positive definite iff every pivot is positive
    double L[3][3] = {};
    for (int j = 0; j < 3; ++j) {
        double d = S[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0)) return VISFS_BA_ERR_BAD_ARGUMENT;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 3; ++i) {
            double t = S[i][j];
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    // S^-1 column by column: L y = e_k, L^T x = y
    double inv[3][3];
    for (int k = 0; k < 3; ++k) {
        double y[3], x[3];
        for (int i = 0; i < 3; ++i) {
            double t = i == k ? 1.0 : 0.0;
            for (int q = 0; q < i; ++q) t -= L[i][q] * y[q];
            y[i] = t / L[i][i];
        }
        for (int i = 2; i >= 0; --i) {
            double t = y[i];
            for (int q = i + 1; q < 3; ++q) t -= L[q][i] * x[q];
            x[i] = t / L[i][i];
        }
        for (int i = 0; i < 3; ++i) inv[i][k] = x[i];
    }
    double info[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) info[3 * a + b] = 0.5 * (inv[a][b] + inv[b][a]);
    if (!finite_all(info, 9)) return VISFS_BA_ERR_BAD_ARGUMENT;
    for (int i = 0; i < 9; ++i) information_out[i] = info[i];
    z_out[0] = T[3]; z_out[1] = T[7]; z_out[2] = std::atan2(T[4], T[0]);
    out_of_plane[0] = T[11];
    out_of_plane[1] = std::atan2(T[9], T[10]);                                             // roll
    out_of_plane[2] = std::atan2(-T[8], std::sqrt(T[0] * T[0] + T[4] * T[4]));             // pitch
    return VISFS_BA_OK;
}

}  // extern "C"
