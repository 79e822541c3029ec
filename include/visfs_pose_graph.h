/*
 * visfs_pose_graph.h — a 2-D pose graph over the loop-closure constraints (implemented in libvisfs_ba_hip.so).
 *
 * The vertices are planar poses (x, y, yaw), the edges relative poses with a 3 x 3 information matrix: the odometry chain and the
 * closures that visfs_scan_group_match_refine (visfs_scan_refine.h) hands out.  Levenberg-Marquardt on all free vertices; the
 * damped normal equations are solved by conjugate gradients preconditioned with the block-tridiagonal part of the matrix (the chain),
 * applied by parallel cyclic reduction.  One workgroup of VISFS_POSE_GRAPH_LANES work items runs the whole optimisation of one
 * graph inside one launch; a one-core host twin (a NULL handle at creation) gives the same bytes.  DESIGN.md section 9p states the
 * residual, the control and every reduction order.
 *
 * Error codes are the VISFS_BA_* of visfs_ba.h.
 */
#ifndef VISFS_POSE_GRAPH_H
#define VISFS_POSE_GRAPH_H

#include <stdint.h>
#include "visfs_ba.h"
#include "visfs_scan_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VISFS_POSE_GRAPH_ABI_VERSION 1

#define VISFS_POSE_GRAPH_LANES 1024                 /* the workgroup size; part of the definition: the sums are formed per lane */
#define VISFS_POSE_GRAPH_MAX_VERTICES 4096          /* N (beyond: VISFS_BA_ERR_UNSUPPORTED) */
#define VISFS_POSE_GRAPH_MAX_EDGES 65536            /* E */
#define VISFS_POSE_GRAPH_MAX_ITERATIONS 50          /* max_iterations outside [1, 50]: VISFS_BA_ERR_BAD_ARGUMENT */
#define VISFS_POSE_GRAPH_MAX_TRIALS 500             /* 10 trials per iteration at most */
#define VISFS_POSE_GRAPH_MAX_ROTATION 1.0           /* |yaw - initial yaw| a trial may reach, radians */
#define VISFS_POSE_GRAPH_TRACE_ITEMS 4              /* per trial: cost, lambda, accepted, PCG iterations */

/* termination */
#define VISFS_POSE_GRAPH_ITERATIONS 0               /* max_iterations outer iterations ran */
#define VISFS_POSE_GRAPH_NO_PROGRESS 1              /* ten trials rejected in a row, or a trial that changed nothing (rho == 0) */
#define VISFS_POSE_GRAPH_TOLERANCE 2                /* an accepted step lowered the cost by function_tolerance of it or less */
#define VISFS_POSE_GRAPH_ROTATION_BOUND 3           /* NO_PROGRESS or TOLERANCE, with a trial of the last iteration rejected for the
                                                       rotation bound: call again from the returned poses */
#define VISFS_POSE_GRAPH_PCG_BUDGET 4               /* the call's PCG iterations reached pcg_budget: the poses accepted so far */

typedef struct visfs_pose_graph visfs_pose_graph;

typedef struct visfs_pose_graph_params {
    double  function_tolerance;            /* default 1e-6; 0: no such test */
    double  pcg_tolerance;                 /* default 1e-8: stop at r.z <= pcg_tolerance^2 * r0.z0 */
    int32_t max_iterations;                /* default 20, 1 .. 50 */
    int32_t max_pcg_iterations;            /* default 500, >= 1: per linear solve; the iterate reached is the step */
    int32_t pcg_budget;                    /* default 10000, >= 1: per call */
    int32_t preconditioner;                /* default 1: block-tridiagonal by cyclic reduction; 0: block-Jacobi */
} visfs_pose_graph_params;

typedef struct visfs_pose_graph_edge {
    int32_t i, j;                          /* vertex indices, i != j */
    double  z[3];                          /* the pose of j in the frame of i: (x, y, yaw) */
    double  information[9];                /* row-major, symmetric (to 1e-12 of its largest entry), positive semi-definite */
    double  huber_delta;                   /* 0: no robust kernel; else on sqrt(chi2), g2o's form */
} visfs_pose_graph_edge;

typedef struct visfs_pose_graph_result {
    int32_t status;                        /* VISFS_BA_OK */
    int32_t iterations, trials;            /* outer iterations run, trials judged (accepted and rejected) */
    int32_t termination;                   /* VISFS_POSE_GRAPH_* */
    int32_t pcg_iterations;                /* of the whole call */
    int32_t free_vertices;                 /* n */
    double  initial_cost, final_cost;      /* the sum of the (robustified) chi2 at the start and at the returned poses */
} visfs_pose_graph_result;

int  visfs_pose_graph_abi_version(void);
void visfs_pose_graph_default_params(visfs_pose_graph_params* p);

/* h: the device and stream of a visfs_ba handle; NULL: the one-core host twin.  max_vertices in 1 .. 4096 and max_edges in
 * 1 .. 65536 size the buffers (beyond: VISFS_BA_ERR_UNSUPPORTED). */
int  visfs_pose_graph_create(visfs_ba_handle* h, int32_t max_vertices, int32_t max_edges, visfs_pose_graph** out);
void visfs_pose_graph_destroy(visfs_pose_graph* pg);
const char* visfs_pose_graph_last_error(const visfs_pose_graph* pg);

/* Optimises the n_vertices poses [N][3] under the edges.  fixed[N]: non-zero holds a vertex; at least one must be held.  A
 * non-finite pose, measurement or information, an asymmetric or indefinite information, a negative huber_delta, an index out of
 * range, i == j, no fixed vertex, a free vertex without any edge or a parameter out of range: VISFS_BA_ERR_BAD_ARGUMENT.  N or E
 * above what the object was created for: VISFS_BA_ERR_UNSUPPORTED.  All of this is decided before anything is pushed; an error
 * leaves the outputs and the hook data of the last call.  poses_out [N][3] (yaw = initial yaw + the rotation found, not wrapped),
 * chi2_out [E] (e^T Omega e at the returned poses, before the robust kernel; may be NULL). */
int  visfs_pose_graph_optimize(visfs_pose_graph* pg, const visfs_pose_graph_params* params, int32_t n_vertices, const double* poses_in,
                               const uint8_t* fixed, int32_t n_edges, const visfs_pose_graph_edge* edges, double* poses_out,
                               double* chi2_out, visfs_pose_graph_result* result);

/* ---- hooks (tests) ----------------------------------------------------------------------------------------------------------- */
/* The trials of the last successful optimize: *trials, and per trial (cost of the trial poses, its lambda, 1 if accepted else 0,
 * PCG iterations of its solve) in order.  A trial that could not be formed or left the rotation bound has the cost DBL_MAX. */
int  visfs_pose_graph_download_trace(visfs_pose_graph* pg, int32_t cap, double* trace /*[cap][4]*/, int32_t* trials);
/* One linearisation at the given poses, no step: per edge (H_ii, H_ij, H_jj) row-major with the robust weight [E][27]; per free row
 * (vertex order) the gradient g [n][3], the diagonal block D [n][9] and the block C towards the next row [n][9] (zero on the last);
 * the cost; chi2 [E].  *n_rows gets n.  Any output may be NULL. */
int  visfs_pose_graph_linearize(visfs_pose_graph* pg, int32_t n_vertices, const double* poses, const uint8_t* fixed, int32_t n_edges,
                                const visfs_pose_graph_edge* edges, int32_t* n_rows, double* edge_blocks, double* g, double* D, double* C,
                                double* cost, double* chi2);
/* z = M^-1 r at the given poses with M the preconditioner of `preconditioner` on H + lambda I; r and z [n][3].
 * VISFS_BA_ERR_SINGULAR when a pivot is not positive. */
int  visfs_pose_graph_precondition(visfs_pose_graph* pg, int32_t preconditioner, double lambda, int32_t n_vertices, const double* poses,
                                   const uint8_t* fixed, int32_t n_edges, const visfs_pose_graph_edge* edges, const double* r, double* z);
/* The host plan of a graph, which needs no object and no device: the checks of optimize (poses aside) and the lists.  *n_rows = n;
 * row_of [N] (-1: fixed); inc_ptr [n + 1] and inc: row r's edges in increasing edge index as 2 * edge + (1 when the row is the
 * edge's j); chain_ptr [n + 1] and chain: the edges that link row r to row r + 1 as 2 * edge + (1 when row r is the edge's j).
 * Room: row_of N, inc_ptr and chain_ptr N + 1, inc 2 E, chain E. */
int  visfs_pose_graph_plan(int32_t n_vertices, const uint8_t* fixed, int32_t n_edges, const visfs_pose_graph_edge* edges, int32_t* n_rows,
                           int32_t* row_of, int32_t* inc_ptr, int32_t* inc, int32_t* chain_ptr, int32_t* chain);
/* launches, copies and waits of the last optimize (0, 0, 0 on the twin) */
int  visfs_pose_graph_last_counts(const visfs_pose_graph* pg, int32_t* launches, int32_t* copies, int32_t* waits);

/* ---- host-only helper --------------------------------------------------------------------------------------------------------- */
/* The edge of a refined scan match: `anchor_pose` (x, y, yaw) is the vertex i the constraint hangs on, `r` the refinement of the
 * scan of vertex j in the same frame.  z = anchor^-1 o (r->x, r->y, r->yaw); information = blkdiag(R^T, 1) r->information
 * blkdiag(R, 1) with R the anchor's rotation, symmetrised.  VISFS_BA_ERR_BAD_ARGUMENT for a NULL or non-finite input or a record
 * with refined == 0. */
int  visfs_pose_graph_edge_from_refine(const double anchor_pose[3], const visfs_scan_refine_result* r, double z_out[3], double information_out[9]);

#ifdef __cplusplus
}
#endif
#endif
