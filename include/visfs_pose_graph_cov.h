/*
 * visfs_pose_graph_cov.h — marginal and relative covariances of the 2-D pose graph (implemented in libvisfs_ba_hip.so).
 *
 * Sigma = H^-1 with H = sum_e w_e J_e^T Omega_e J_e at the poses handed in, over the free vertices in the row order of
 * visfs_pose_graph_plan: w_e is the Huber weight at those poses and there is no damping, so H is what visfs_pose_graph_linearize
 * returns.  The blocks of a fixed vertex are zero.  A call answers up to VISFS_POSE_GRAPH_COV_MAX_QUERIES pairs (a, b) of vertices:
 * the 6 x 6 joint covariance of the two poses and the first-order covariance of a^-1 o b, which is what the search window of a
 * loop-closure candidate (visfs_scan_group_match_refine) is made from.
 *
 * Every column of Sigma that a query needs is one linear solve H x = e by the conjugate gradients of visfs_pose_graph.h, with the
 * same preconditioner and the same lane sums; a column is one workgroup and no workgroup waits for another.  The one-core host
 * twin (an object created with a NULL handle) runs the columns in a loop and returns the same bytes.  DESIGN.md section 9q.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_POSE_GRAPH_COV_H
#define VISFS_POSE_GRAPH_COV_H

#include <stdint.h>
#include "visfs_pose_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_POSE_GRAPH_COV_ABI_VERSION 1

#define VISFS_POSE_GRAPH_COV_MAX_QUERIES 1024       /* Q outside [1, 1024]: VISFS_BA_ERR_BAD_ARGUMENT */
#define VISFS_POSE_GRAPH_COV_MAX_SOURCES 64         /* distinct free vertices among the queries (beyond: VISFS_BA_ERR_UNSUPPORTED) */

typedef struct visfs_pose_graph_cov_params {
    double  pcg_tolerance;                 /* default 1e-8: a column stops at r.z <= pcg_tolerance^2 * r0.z0 */
    int32_t max_pcg_iterations;            /* default 500, >= 1: per column; the iterate reached is used */
    int32_t preconditioner;                /* default 1: block-tridiagonal by cyclic reduction; 0: block-Jacobi */
} visfs_pose_graph_cov_params;

typedef struct visfs_pose_graph_cov_result {
    int32_t status;                        /* VISFS_BA_OK */
    int32_t sources;                       /* distinct free vertices among the queries */
    int32_t columns;                       /* 3 * sources linear solves */
    int32_t pcg_iterations_max;            /* of the slowest column */
    int32_t pcg_iterations_total;          /* of all columns */
    int32_t unconverged_columns;           /* columns that ran max_pcg_iterations iterations */
    int32_t free_vertices;                 /* n */
    int32_t reserved;
    double  cost;                          /* the sum of the (robustified) chi2 at the poses handed in */
} visfs_pose_graph_cov_result;

int  visfs_pose_graph_cov_abi_version(void);
void visfs_pose_graph_cov_default_params(visfs_pose_graph_cov_params* p);

/* The covariances of n_queries pairs of vertices, queries [Q][2] = (a, b); a == b and fixed vertices are allowed.
 *   joint_out [Q][36]:   the covariance of (x_a, y_a, yaw_a, x_b, y_b, yaw_b), row-major, symmetric.
 *   relative_out [Q][9]: the covariance of z = a^-1 o b to first order, [J_i J_j] joint [J_i J_j]^T with the derivatives of an
 *                        edge i = a, j = b at the poses handed in.
 * Either may be NULL.  Everything visfs_pose_graph_optimize refuses is refused here in the same way; moreover a query index out of
 * range, Q outside [1, 1024] or a parameter out of range: VISFS_BA_ERR_BAD_ARGUMENT; more than 64 distinct free vertices among the
 * queries: VISFS_BA_ERR_UNSUPPORTED; a free vertex that no path of edges links to a fixed vertex: VISFS_BA_ERR_SINGULAR (Sigma does
 * not exist).  All of this is decided before anything is pushed.  A pivot of the preconditioner that is not positive, or conjugate
 * gradients that break down (p^T H p not positive or not finite): VISFS_BA_ERR_SINGULAR, the outputs are not written.  A column
 * that ran max_pcg_iterations iterations is counted in unconverged_columns and its iterate is used.  The call leaves the trace and
 * the counts of the object's last visfs_pose_graph_optimize as they were. */
int  visfs_pose_graph_covariance(visfs_pose_graph* pg, const visfs_pose_graph_cov_params* params, int32_t n_vertices, const double* poses,
                                 const uint8_t* fixed, int32_t n_edges, const visfs_pose_graph_edge* edges, int32_t n_queries,
                                 const int32_t* queries, double* joint_out, double* relative_out, visfs_pose_graph_cov_result* result);

/* ---- hooks (tests) ----------------------------------------------------------------------------------------------------------- */
/* The three solved columns of source `source` of the last successful covariance call, columns [3][n][3] (column, row, coordinate),
 * and their iteration counts [3].  Either may be NULL. */
int  visfs_pose_graph_cov_download_columns(visfs_pose_graph* pg, int32_t source, double* columns, int32_t* iterations);
/* The host plan of a covariance call, which needs no object and no device: the checks (poses aside), the sources (vertex indices in
 * order of first appearance, a before b) and per query the indices of its two sources (-1 for a fixed vertex).
 * Room: sources 64, query_sources 2 Q. */
int  visfs_pose_graph_cov_plan(int32_t n_vertices, const uint8_t* fixed, int32_t n_edges, const visfs_pose_graph_edge* edges, int32_t n_queries,
                               const int32_t* queries, int32_t* n_sources, int32_t* sources, int32_t* query_sources);
/* launches, copies and waits of the last covariance call (0, 0, 0 on the twin) */
int  visfs_pose_graph_cov_last_counts(const visfs_pose_graph* pg, int32_t* launches, int32_t* copies, int32_t* waits);

/* ---- host-only helper --------------------------------------------------------------------------------------------------------- */
/* The search window of a loop-closure candidate from relative[9]: linear = sigmas * sqrt(the larger eigenvalue of the x, y block),
 * angular = sigmas * sqrt(relative[8]).  VISFS_BA_ERR_BAD_ARGUMENT for a NULL or non-finite input, a negative variance or a
 * negative sigmas. */
int  visfs_pose_graph_cov_search_window(const double relative[9], double sigmas, double* linear, double* angular);

#ifdef __cplusplus
}
#endif
#endif
