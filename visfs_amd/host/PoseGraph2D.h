// PoseGraph2D.h — VISFS::PoseGraph2D: the 2-D pose graph of include/visfs_pose_graph.h as a container.  Vertices and edges are added
// as the trajectory grows (addVertex, addEdge), a loop closure comes in as the refinement record of VISFS::ScanStackGroup::matchRefine
// with the pose of the vertex it hangs on (addClosure), and optimize() runs the solver: on the device of a visfs_ba handle, or on
// the one-core host twin without one.  A call that ends at the rotation bound is repeated from the poses it returned (the anchor of
// the yaw polynomial moves there), so a caller never sees VISFS_POSE_GRAPH_ROTATION_BOUND unless maxCalls runs out.
// covariance() answers pairs of vertices with their joint and relative covariances at the poses held (include/visfs_pose_graph_cov.h),
// searchWindow(i, j, sigmas) turns one of them into the two windows of a loop-closure search of the scan of j against the sub-map of i.
// Header-only; link libvisfs_ba_hip.so.
#ifndef VISFS_POSE_GRAPH_2D_H
#define VISFS_POSE_GRAPH_2D_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "visfs_pose_graph.h"
#include "visfs_pose_graph_cov.h"

namespace VISFS {

class PoseGraph2D {
public:
    struct Summary {
        int status = VISFS_BA_OK, calls = 0, iterations = 0, trials = 0, pcgIterations = 0, termination = 0;
        double initialCost = 0.0, finalCost = 0.0;
    };

    struct Covariance {
        int status = VISFS_BA_OK;
        visfs_pose_graph_cov_result result{};
        std::vector<double> joint, relative;      // [Q][36], [Q][9]
    };

    // ba == nullptr: the host twin
    explicit PoseGraph2D(visfs_ba_handle* ba, int maxVertices = VISFS_POSE_GRAPH_MAX_VERTICES, int maxEdges = VISFS_POSE_GRAPH_MAX_EDGES) {
        const int rc = visfs_pose_graph_create(ba, maxVertices, maxEdges, &pg_);
        if (rc != VISFS_BA_OK) throw std::runtime_error("visfs_pose_graph_create failed with status " + std::to_string(rc));
        visfs_pose_graph_default_params(&params_);
        visfs_pose_graph_cov_default_params(&covParams_);
    }
    ~PoseGraph2D() { visfs_pose_graph_destroy(pg_); }
    PoseGraph2D(const PoseGraph2D&) = delete;
    PoseGraph2D& operator=(const PoseGraph2D&) = delete;

    visfs_pose_graph_params& params() { return params_; }
    visfs_pose_graph_cov_params& covParams() { return covParams_; }

    int addVertex(double x, double y, double yaw, bool fixed = false) {
        poses_.insert(poses_.end(), { x, y, yaw });
        fixed_.push_back(fixed ? 1 : 0);
        return (int)fixed_.size() - 1;
    }

    // z: the pose of j in the frame of i; information row-major 3 x 3
    void addEdge(int i, int j, const double z[3], const double information[9], double huberDelta = 0.0) {
        visfs_pose_graph_edge e{};
        e.i = i; e.j = j; e.huber_delta = huberDelta;
        for (int k = 0; k < 3; ++k) e.z[k] = z[k];
        for (int k = 0; k < 9; ++k) e.information[k] = information[k];
        edges_.push_back(e);
    }

    // The closure of a scan taken at vertex j, refined against a sub-map whose frame is that of `anchorPose`, the pose of vertex i.
    int addClosure(int i, int j, const visfs_scan_refine_result& refined, const double anchorPose[3], double huberDelta = 0.0) {
        double z[3], W[9];
        const int rc = visfs_pose_graph_edge_from_refine(anchorPose, &refined, z, W);
        if (rc == VISFS_BA_OK) addEdge(i, j, z, W, huberDelta);
        return rc;
    }

    int numVertices() const { return (int)fixed_.size(); }
    int numEdges() const { return (int)edges_.size(); }
    const double* pose(int i) const { return poses_.data() + 3 * (size_t)i; }
    const std::vector<double>& chi2() const { return chi2_; }

    // Optimises the poses in place; at most maxCalls solver calls, a new one after each that ended at the rotation bound.
    Summary optimize(int maxCalls = 8) {
        Summary s;
        std::vector<double> out(poses_.size());
        chi2_.assign(edges_.size(), 0.0);
        for (int c = 0; c < maxCalls; ++c) {
            visfs_pose_graph_result r{};
            s.status = visfs_pose_graph_optimize(pg_, &params_, numVertices(), poses_.data(), fixed_.data(), numEdges(), edges_.data(), out.data(),
                                                 chi2_.data(), &r);
            if (s.status != VISFS_BA_OK) return s;
            poses_ = out;
            if (c == 0) s.initialCost = r.initial_cost;
            ++s.calls; s.iterations += r.iterations; s.trials += r.trials; s.pcgIterations += r.pcg_iterations;
            s.finalCost = r.final_cost; s.termination = r.termination;
            if (r.termination != VISFS_POSE_GRAPH_ROTATION_BOUND) break;
        }
        return s;
    }

    // The joint and relative covariances of pairs (a, b) of vertices at the poses held; at most 64 distinct free vertices a call.
    Covariance covariance(const std::vector<std::pair<int, int>>& queries) {
        Covariance c;
        std::vector<int32_t> q;
        for (const auto& p : queries) { q.push_back(p.first); q.push_back(p.second); }
        c.joint.assign(36 * queries.size(), 0.0);
        c.relative.assign(9 * queries.size(), 0.0);
        c.status = visfs_pose_graph_covariance(pg_, &covParams_, numVertices(), poses_.data(), fixed_.data(), numEdges(), edges_.data(),
                                               (int32_t)queries.size(), q.data(), c.joint.data(), c.relative.data(), &c.result);
        return c;
    }

    // The windows of a search for the scan of vertex j in the sub-map anchored at vertex i: `sigmas` standard deviations of the
    // relative pose i^-1 o j, in metres and radians (linear_search_window and angular_search_window of visfs_scan_group_match_refine).
    int searchWindow(int i, int j, double sigmas, double* linear, double* angular) {
        const Covariance c = covariance({ { i, j } });
        if (c.status != VISFS_BA_OK) return c.status;
        return visfs_pose_graph_cov_search_window(c.relative.data(), sigmas, linear, angular);
    }

    void covLastCounts(int* launches, int* copies, int* waits) const {
        int32_t a = 0, b = 0, c = 0;
        visfs_pose_graph_cov_last_counts(pg_, &a, &b, &c);
        if (launches) *launches = a;
        if (copies) *copies = b;
        if (waits) *waits = c;
    }

    void lastCounts(int* launches, int* copies, int* waits) const {
        int32_t a = 0, b = 0, c = 0;
        visfs_pose_graph_last_counts(pg_, &a, &b, &c);
        if (launches) *launches = a;
        if (copies) *copies = b;
        if (waits) *waits = c;
    }
    const char* lastError() const { return visfs_pose_graph_last_error(pg_); }

private:
    visfs_pose_graph* pg_ = nullptr;
    visfs_pose_graph_params params_{};
    visfs_pose_graph_cov_params covParams_{};
    std::vector<double> poses_, chi2_;
    std::vector<uint8_t> fixed_;
    std::vector<visfs_pose_graph_edge> edges_;
};

}  // namespace VISFS

#endif
