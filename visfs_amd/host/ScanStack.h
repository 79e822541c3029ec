// ScanStack.h — a frozen sub-map grid with its window-maximum levels, searched by branch and bound (include/visfs_scan_fast.h):
// relocalisation in a known map and loop closure against a finished sub-map.  Header only, over the C ABI.
//
// A ScanStack comes from ActiveSubmaps2D::freeze (a snapshot of a live sub-map: later insertions do not change it) or from a saved
// grid (fromGrid: the cells and limits ActiveSubmaps2D::download and submaps() hand out).  A device stack runs on the stream of the
// handle it was made on, which must outlive it.
//
// A ScanStackGroup (include/visfs_scan_group.h) matches one scan against several stacks in one call: the candidate sub-maps of a loop
// closure, or every sub-map of a saved map.  On the device its launches, copies and waits do not grow with the number of stacks.
//
// refine / matchRefine (include/visfs_scan_refine.h) take a matched pose off the search lattice: the continuous refinement of the
// occupied-space cost on the same grid, with a pull towards a target translation and the start's yaw.
#ifndef VISFS_AMD_SCAN_STACK_H
#define VISFS_AMD_SCAN_STACK_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "visfs_scan_fast.h"
#include "visfs_scan_group.h"
#include "visfs_scan_refine.h"

namespace VISFS {

// A refined pose with the 3 x 3 information matrix (J^T J, row-major over x, y, yaw) of the constraint it stands for.
struct RefinedPose {
    double x = 0.0, y = 0.0, yaw = 0.0, initialCost = 0.0, finalCost = 0.0;
    double information[9] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int iterations = 0;
    bool refined = false;                     // false: nothing to refine (no returns, no sub-map yet, a skipped member): the start back
    static RefinedPose from(const visfs_scan_refine_result& r) {
        RefinedPose o;
        o.x = r.x; o.y = r.y; o.yaw = r.yaw; o.initialCost = r.initial_cost; o.finalCost = r.final_cost;
        for (int i = 0; i < 9; ++i) o.information[i] = r.information[i];
        o.iterations = r.iterations; o.refined = r.refined != 0;
        return o;
    }
};

class ScanStack {
public:
    ScanStack() = default;
    explicit ScanStack(visfs_scan_stack* st) : st_(st) {}                 // takes ownership
    ScanStack(const ScanStack&) = delete;
    ScanStack& operator=(const ScanStack&) = delete;
    ScanStack(ScanStack&& o) noexcept : st_(o.st_) { o.st_ = nullptr; }
    ScanStack& operator=(ScanStack&& o) noexcept { if (this != &o) { visfs_scan_stack_destroy(st_); st_ = o.st_; o.st_ = nullptr; } return *this; }
    ~ScanStack() { visfs_scan_stack_destroy(st_); }

    // From a saved grid: cells [num_y_cells][num_x_cells].  ba == nullptr: the one-core host twin.  Throws when creation fails.
    static ScanStack fromGrid(visfs_ba_handle* ba, const visfs_submap_info& limits, const std::vector<uint16_t>& cells, int depth = 7) {
        if (limits.num_x_cells < 1 || limits.num_y_cells < 1 || cells.size() != (size_t)limits.num_x_cells * (size_t)limits.num_y_cells)
            throw std::runtime_error("ScanStack::fromGrid: the cells do not fit the limits");
        visfs_scan_stack* st = nullptr;
        const int rc = visfs_scan_stack_create_from_grid(ba, &limits, cells.data(), depth, &st);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_scan_stack_create_from_grid failed with status " + std::to_string(rc));
        return ScanStack(st);
    }

    bool valid() const { return st_ != nullptr; }
    visfs_scan_stack* get() const { return st_; }
    visfs_scan_stack_info info() const { visfs_scan_stack_info i{}; visfs_scan_stack_describe(st_, &i); return i; }

    // The pose guess (x, y, yaw) corrected by the search of the returns (robot frame, xyz triples) within the windows of `params`
    // (default: 7 m, 30 degrees).  matched is false when the best score lies below params->min_score, or without returns.
    struct Match { double x = 0.0, y = 0.0, yaw = 0.0, score = 0.0; bool matched = false; };
    int match(const double guess[3], const std::vector<double>& returns, Match* out, const visfs_scan_stack_params* params = nullptr,
              visfs_scan_stack_result* full = nullptr) const {
        visfs_scan_stack_params p;
        if (params) p = *params; else visfs_scan_stack_default_params(&p);
        visfs_scan_stack_result r;
        const int rc = visfs_scan_stack_match(st_, &p, guess, (int32_t)(returns.size() / 3), returns.data(), &r);
        if (rc != VISFS_BA_OK) return rc;
        if (out) { out->x = r.match.x; out->y = r.match.y; out->yaw = r.match.yaw; out->score = r.match.score; out->matched = r.match.matched != 0; }
        if (full) *full = r;
        return rc;
    }

    // The pose `initial` (x, y, yaw; a match's winner) refined on the grid's level 0 towards the translation `target` (x, y; the
    // prediction).  params == nullptr: Cartographer's weights 1, 10, 40.
    int refine(const double initial[3], const double target[2], const std::vector<double>& returns, RefinedPose* out,
               const visfs_scan_refine_params* params = nullptr, visfs_scan_refine_result* full = nullptr) const {
        visfs_scan_refine_params p;
        if (params) p = *params; else visfs_scan_refine_default_params(&p);
        visfs_scan_refine_result r;
        const int rc = visfs_scan_stack_refine(st_, &p, initial, target, (int32_t)(returns.size() / 3), returns.data(), &r);
        if (rc != VISFS_BA_OK) return rc;
        if (out) *out = RefinedPose::from(r);
        if (full) *full = r;
        return rc;
    }

    const char* lastError() const { return visfs_scan_stack_last_error(st_); }

private:
    visfs_scan_stack* st_ = nullptr;
};

// Several stacks of one flavour (device stacks of one handle, or host twins) with equal resolution and depth, searched in one call.
// The stacks must outlive the group; a stack may be in several groups.
class ScanStackGroup {
public:
    // Throws std::runtime_error when creation fails; the text names the offending member.
    explicit ScanStackGroup(const std::vector<const ScanStack*>& stacks) {
        std::vector<visfs_scan_stack*> m;
        for (const ScanStack* s : stacks) m.push_back(s ? s->get() : nullptr);
        const int rc = visfs_scan_group_create((int32_t)m.size(), m.data(), &g_);
        if (rc != VISFS_BA_OK)
            throw std::runtime_error("visfs_scan_group_create failed with status " + std::to_string(rc) + ": " + visfs_scan_group_last_error(nullptr));
        m_ = m.size();
    }
    ScanStackGroup(const ScanStackGroup&) = delete;
    ScanStackGroup& operator=(const ScanStackGroup&) = delete;
    ~ScanStackGroup() { visfs_scan_group_destroy(g_); }

    size_t size() const { return m_; }

    // One member's outcome: ok is false when its frontier overflowed (the other fields are then not filled).
    struct Match : ScanStack::Match { bool ok = false; int32_t sum = 0; };
    // The returns (robot frame, xyz triples) against every member, each about its own guess (guesses: [size()][3]).  `best` gets the
    // matched member of the largest sum (the lowest index among equal sums), or -1.
    int match(const std::vector<double>& guesses, const std::vector<double>& returns, std::vector<Match>* out, int* best,
              const visfs_scan_stack_params* params = nullptr, std::vector<visfs_scan_stack_result>* full = nullptr) const {
        if (guesses.size() != 3 * m_) return VISFS_BA_ERR_BAD_ARGUMENT;
        visfs_scan_stack_params p;
        if (params) p = *params; else visfs_scan_stack_default_params(&p);
        std::vector<visfs_scan_stack_result> r(m_);
        std::vector<int32_t> status(m_);
        int32_t b = -1;
        const int rc = visfs_scan_group_match(g_, &p, guesses.data(), (int32_t)(returns.size() / 3), returns.data(), r.data(), status.data(), &b);
        if (rc != VISFS_BA_OK) return rc;
        if (out) {
            out->assign(m_, Match());
            for (size_t i = 0; i < m_; ++i) {
                if (status[i] != VISFS_BA_OK) continue;
                Match& o = (*out)[i];
                o.ok = true; o.x = r[i].match.x; o.y = r[i].match.y; o.yaw = r[i].match.yaw; o.score = r[i].match.score; o.sum = r[i].match.sum;
                o.matched = r[i].match.matched != 0;
            }
        }
        if (best) *best = b;
        if (full) *full = r;
        return rc;
    }

    // match, and in the same call every matched member's winner refined towards its guess's translation (refined[i].refined is false
    // for a member that overflowed or stayed below min_score).  On the device: one launch more than match.
    int matchRefine(const std::vector<double>& guesses, const std::vector<double>& returns, std::vector<Match>* out, int* best,
                    std::vector<RefinedPose>* refined, const visfs_scan_stack_params* params = nullptr,
                    const visfs_scan_refine_params* refineParams = nullptr, std::vector<visfs_scan_stack_result>* full = nullptr) const {
        if (guesses.size() != 3 * m_) return VISFS_BA_ERR_BAD_ARGUMENT;
        visfs_scan_stack_params p;
        if (params) p = *params; else visfs_scan_stack_default_params(&p);
        visfs_scan_refine_params q;
        if (refineParams) q = *refineParams; else visfs_scan_refine_default_params(&q);
        std::vector<visfs_scan_stack_result> r(m_);
        std::vector<visfs_scan_refine_result> f(m_);
        std::vector<int32_t> status(m_);
        int32_t b = -1;
        const int rc = visfs_scan_group_match_refine(g_, &p, &q, guesses.data(), (int32_t)(returns.size() / 3), returns.data(), r.data(), status.data(), &b,
                                                     f.data());
        if (rc != VISFS_BA_OK) return rc;
        if (out) {
            out->assign(m_, Match());
            for (size_t i = 0; i < m_; ++i) {
                if (status[i] != VISFS_BA_OK) continue;
                Match& o = (*out)[i];
                o.ok = true; o.x = r[i].match.x; o.y = r[i].match.y; o.yaw = r[i].match.yaw; o.score = r[i].match.score; o.sum = r[i].match.sum;
                o.matched = r[i].match.matched != 0;
            }
        }
        if (refined) {
            refined->clear();
            for (size_t i = 0; i < m_; ++i) refined->push_back(RefinedPose::from(f[i]));
        }
        if (best) *best = b;
        if (full) *full = r;
        return rc;
    }

    // what the last match issued on the device (all zero for host twins)
    void lastCounts(int* launches, int* copies, int* synchronisations) const {
        int32_t k = 0, c = 0, s = 0;
        visfs_scan_group_last_counts(g_, &k, &c, &s);
        if (launches) *launches = k;
        if (copies) *copies = c;
        if (synchronisations) *synchronisations = s;
    }

    const char* lastError() const { return visfs_scan_group_last_error(g_); }

private:
    visfs_scan_group* g_ = nullptr;
    size_t m_ = 0;
};

}  // namespace VISFS

#endif
