/*
 * okx.h — C-ABI of the MI355X-native batched suspension-kinematics constraint solver.
 *
 * This is the drop-in boundary for ONE hot path of nickmccleery/open-kinematics: the
 * per-sweep-step nonlinear least-squares solve.  The reference has no FFI for this path
 * (it is pure Python); the entry points below are what a binding for it would bind, and
 * each cites the reference interface it replaces (paths relative to the reference root,
 * src/kinematics/core/...).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*.
 *   - every pointer named d_* is a DEVICE-ACCESSIBLE pointer: normally HBM; pinned host
 *     memory (hipHostMalloc / hipHostRegister, mapped) is accepted as well - okx_solve_batch's
 *     d_targets, d_out_pos and d_info then cross PCIe as the kernel reads / stores them, with
 *     no copy command on either side (bench.py `e2e.zero_copy`; the host may read the outputs
 *     once an event recorded after the call has completed).  Everything else is host memory
 *     that is only read during the call.
 *   - all entry points return OKX_OK (0) or a negative okx_status; they never throw.
 *     okx_last_error() returns a thread-local message for the last failure.
 *   - all floating point is IEEE fp64; lengths in millimetres, angles in radians.
 *
 * The "constraint program" is the flattened form of what the reference passes to
 * solve_suspension_sweep() (solver.py:654-660): initial SuspensionState (state.py:23-72),
 * list[Constraint] (constraints.py), DerivedPointsManager spec (points/derived/) and the
 * target rows of a SweepConfig (targeting.py:51-104).
 */
#ifndef OKX_H
#define OKX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OKX_ABI_VERSION 6   /* okx_diagnose_sweeps_batch (sweep diagnostics on device: okx_diag_roles, okx_diag_summary, okx_diag_issue) was ADDED UNDER 6 - nothing existing changed; a caller that must know whether a library has it looks the symbol up (dlsym).  6: the evaluated solve of composed axles (okx_axle_roles, okx_program_enable_axle_evaluation, okx_precompile_axle_evaluation, okx_program_eval_columns).  5: the evaluated solve (okx_program_enable_evaluation, okx_solve_evaluated_batch, okx_evaluate_batch, okx_precompile_evaluation).  4: okx_rotation_role.kind / point_b (hardware metrics of composed axles), okx_program_has_cold_body, okx_program_ready.  3: okx_solve_opts.output (+ reserved); lane kernel entry points.  2: confirm_full_pass; diagnostics moved to okx_debug.h */

/* Hard limits of one problem (one wavefront owns one problem). */
#define OKX_MAX_VARS 126     /* n = 3 * free points (one thread per variable: one wavefront up to 63, two beyond) */
#define OKX_MAX_ROWS 128     /* m = constraint rows + target rows                    */
#define OKX_MAX_POINTS 96    /* fixed + free + derived                               */
#define OKX_MAX_TARGETS 8
#define OKX_ROW_PARAMS 8     /* doubles per constraint row                           */
#define OKX_ROW_POINTS 4     /* point slots per constraint row                       */

typedef enum okx_status {
  OKX_OK = 0,
  OKX_ERR_INVALID = -1,      /* malformed program / argument                         */
  OKX_ERR_LIMIT = -2,        /* exceeds an OKX_MAX_* limit                           */
  OKX_ERR_UNDERDETERMINED = -3, /* n_vars > n_rows (solver.py:116-121)               */
  OKX_ERR_DEVICE = -4,       /* HIP runtime failure (no GPU, launch error, ...)      */
  OKX_ERR_ALLOC = -5
} okx_status;

/*
 * Constraint row types.  One scalar residual per row, defined exactly as
 * constraints.py does (softnorm(s) = sqrt(s + 1e-12) - 1e-6, soft_math.py:16-27);
 * Jacobian rows follow jacobians.py / tools/generate_jacobians.py.
 * Point slots p0..p3 and params q0..q7 per type:
 */
typedef enum okx_row_type {
  OKX_ROW_DISTANCE = 0,          /* constraints.py:89-134   p0=p1,p1=p2        q0=L                */
  OKX_ROW_SPHERICAL = 1,         /* constraints.py:137-170  p0,p1              —                   */
  OKX_ROW_ANGLE = 2,             /* constraints.py:173-243  v1s,v1e,v2s,v2e    q0=alpha            */
  OKX_ROW_THREE_POINT_ANGLE = 3, /* constraints.py:246-308  p1,p2(vertex),p3   q0=alpha            */
  OKX_ROW_VECTORS_PARALLEL = 4,  /* constraints.py:311-371  v1s,v1e,v2s,v2e    —                   */
  OKX_ROW_VECTORS_PERPENDICULAR = 5, /* constraints.py:374-429 same            —                   */
  OKX_ROW_EQUAL_DISTANCE = 6,    /* constraints.py:432-477  p1,p2,p3,p4        —                   */
  OKX_ROW_FIXED_AXIS = 7,        /* constraints.py:480-516  p0                 q0=axis(0/1/2) q1=value */
  OKX_ROW_POINT_ON_LINE = 8,     /* constraints.py:519-576  p0                 q0..2=line point q3..5=line dir */
  OKX_ROW_POINT_ON_PLANE = 9,    /* constraints.py:579-627  p0                 q0..2=plane point q3..5=normal  */
  OKX_ROW_MIDPOINT_ON_PLANE = 10,/* constraints.py:630-666  a,b                q0..2=plane point q3..5=normal  */
  OKX_ROW_COPLANAR = 11,         /* constraints.py:669-709  p1..p4             —                   */
  OKX_ROW_SCALAR_TRIPLE = 12,    /* constraints.py:712-733  p1..p4             q0=V q1=scale       */
  /*
   * Extension (not a reference class): one Cartesian component of
   * cross(p - line_point, line_dir).  Three such rows replace one POINT_ON_LINE row
   * when the host flattens with line_mode="pinned"; sum of squares = d^2 instead of
   * softnorm(d^2)^2.  Same minimiser whenever the point can reach the line;
   * it removes the reference row's zero-gradient degeneracy (sensitivity.py:83-87,146-174
   * does the same with explicit pins).
   */
  OKX_ROW_LINE_PIN = 13,         /* p0  q0..2=line point q3..5=line dir q6=component(0/1/2)        */
  OKX_ROW_TYPE_COUNT = 14
} okx_row_type;

/*
 * Derived-point ops (points/derived/definitions.py), evaluated in the given
 * (topological) order; closed-form 3x3 chain-rule blocks replace the reference's
 * dual-number pass (manager.py:271-324).
 */
typedef enum okx_dop_type {
  OKX_DOP_MIDPOINT = 0,      /* definitions.py:76-89    out = a + (b - a)/2               pts=(a,b)           */
  OKX_DOP_ALONG = 1,         /* definitions.py:24-33,92-155 out = base + normalize(a - b)*c pts=(base,a,b) q=c */
  OKX_DOP_CONTACT_PATCH = 2, /* definitions.py:36-73,158-180 out = wc + normalize(-Z - ((-Z).ax)ax)*R,
                                ax = normalize(axo - axi)   pts=(wc,axi,axo) q=R                              */
  OKX_DOP_TYPE_COUNT = 3
} okx_dop_type;

/* Flattened constraint program (host arrays; copied by okx_program_create). */
typedef struct okx_program_desc {
  int32_t abi_version;        /* = OKX_ABI_VERSION */
  int32_t n_points;           /* P: all points, any order */
  int32_t n_free;             /* F: free points; n_vars = 3F */
  int32_t n_derived;          /* D */
  int32_t n_rows;             /* Mc: constraint rows (targets excluded) */
  int32_t n_targets;          /* T: target rows appended after the constraint rows */
  int32_t n_out;              /* points written per solved problem */
  int32_t reserved;
  const int32_t* free_point;  /* [F]      point index of variable block k (state.py:46-50 order) */
  const int32_t* dop_type;    /* [D]      okx_dop_type */
  const int32_t* dop_out;     /* [D]      output point index */
  const int32_t* dop_pts;     /* [D][4]   input point indices, -1 = unused */
  const double* dop_param;    /* [D]      scalar parameter */
  const int32_t* row_type;    /* [Mc]     okx_row_type */
  const int32_t* row_pts;     /* [Mc][4]  point indices, -1 = unused */
  const double* row_param;    /* [Mc][8]  design-state parameters (geometry 0) */
  const int32_t* tgt_point;   /* [T]      targeted point */
  const double* tgt_dir;      /* [T][3]   unit direction (targeting.py:135-148) */
  const int32_t* out_point;   /* [n_out]  output point indices (Suspension.output_points()) */
  const double* design_pos;   /* [P][3]   design positions incl. derived (geometry 0) */
} okx_program_desc;

typedef struct okx_program okx_program; /* opaque, device-resident */

/* Levenberg–Marquardt controls.  Zero-initialise then call okx_default_opts(). */
typedef struct okx_solve_opts {
  int32_t max_iter;       /* LM iterations per problem (default 100)                       */
  int32_t chain;          /* 0: every problem starts from its geometry's design state
                             (independent problems, one wavefront each);
                             1: reference semantics (solver.py:716,774): problems of one
                             geometry form a sequential chain, step k starts at step k-1's
                             solution; one wavefront walks one chain.                      */
  int64_t steps_per_geometry; /* problems [g*S, (g+1)*S) use geometry g; 0 = single geometry */
  int64_t chain_len;      /* > 0: consecutive problems are grouped into chains of this length
                             (never across geometries); one wavefront walks one chain and
                             warm-starts each problem from its predecessor, the chain head
                             starts from the design state.  1 = independent cold starts,
                             0 = take the length from `chain` (0 -> 1, 1 -> whole sweep),
                             -1 = auto: one chain per resident wavefront.                  */
  double step_tol;        /* stop when max|dx| <= step_tol (mm, default 1e-11)             */
  double grad_tol;        /* > 0: stop when max|J^T r| <= grad_tol.  < 0: MINPACK's gtol (what SolverConfig.gtol means,
                             solver.py:158-169): stop when max_j |(J^T r)_j| / (|J_j| |r|) <= -grad_tol (lmder's gnorm:
                             the cosine between the residual and the Jacobian's columns).  0 (default): unused.  A launch
                             with a gradient stop runs the general bodies without the shared first step. */
  double ftol;            /* stop when an accepted step reduces the cost by <= ftol*cost,
                             actual and predicted (MINPACK's ftol test; default 1e-10):
                             terminates infeasible targets at their compromise point so
                             that the residual_tolerance check can reject them
                             (solver.py:732-747)                                           */
  double lambda0;         /* initial damping relative to max diag(J^T J) (default 1e-6)    */
  double residual_tolerance; /* informational: info.flags bit1 set if max|r| exceeds it
                                (solver.py:735-747, default 1e-3)                          */
  int32_t kernel;         /* 0 auto (the runtime-specialised quad kernel when the program has one,
                             else 1 or 2 by size), 1 generic interpreter, one problem per
                             wavefront, 2 generic lane-group packed (several small problems per
                             wavefront; falls back to 1 when a problem needs more than 32
                             lanes), 3 quad kernel (OKX_ERR_INVALID when the program has none),
                             4 lane kernel (one lane per problem, 64 per wavefront; auto picks it for
                             batches of at least okx_program_lane_threshold() problems)          */
  int32_t confirm_full_pass; /* quad kernel only.  0 (default): a step predicted to land within
                             step_tol of the solution (damping contraction lambda / min pivot and
                             the observed quadratic contraction, both with a 100x margin) is
                             applied and confirmed by a residual-only evaluation (cost must not
                             rise) instead of a full Jacobian / factorisation pass.
                             non-zero: always end on a computed correction <= step_tol.        */
  int32_t predictor;      /* quad kernel, own-geometry launches.  non-zero: chain heads (cold starts) begin at
                             the polynomial model of okx_program_fit_predictor instead of the design state
                             (ignored until a predictor has been fitted).  Same solutions, fewer passes. */
  int32_t shared_first_step; /* quad kernel (single mode).  non-zero (default 1): a chain head starts at its geometry's
                             design state, where only the target residuals depend on the problem: the constraint
                             residuals, the Jacobian, J^T J and its damped factorisation are identical for every problem
                             of that geometry.  That first Levenberg-Marquardt pass is evaluated ONCE PER GEOMETRY (own
                             geometry: once per program and lambda0; geometry tables: a small launch ahead of the solve,
                             when there are at least four steps per geometry) and every head takes its first step
                             dx = -(Q_0 + sum_t r_t Q_t), Q_k = (J^T J + lambda I)^-1 G_k, from that table.  Same
                             iteration, same iterates up to rounding; info.nfev counts the evaluations a problem ran
                             itself.  0: every chain head runs its own first pass.  With geometry tables the scratch
                             table lives in the program: such launches of one program must be stream-ordered.  Own
                             geometry: one table per lambda0, the default's filled at okx_program_create, any other by
                             the first launch that asks for it (on its stream; launches on other streams wait for it). */
  int32_t output;         /* what okx_solve_batch writes to d_out_pos (generated kernels; the interpreter kernels only
                             know OKX_OUTPUT_RECORDS):
                             OKX_OUTPUT_RECORDS (0, default) [B][n_out][3]: every output point, the reference's state copy
                               (solver.py:763);
                             OKX_OUTPUT_FREE [B][n_free][3]: the solved free points only, in the program's free_point order
                               (144 B instead of 360 B per double-wishbone solve: what a PCIe link or an xGMI all-gather
                               wants to carry; okx_expand_positions_batch rebuilds the records, bit-identical);
                             OKX_OUTPUT_NONE: nothing (d_out_pos may be NULL) - only d_info, for feasibility scans.      */
  int32_t reserved;
} okx_solve_opts;

enum { OKX_OUTPUT_RECORDS = 0, OKX_OUTPUT_FREE = 1, OKX_OUTPUT_NONE = 2 };

/* Per-problem result, the device analogue of SolverInfo (solver.py:83-96).
 * max_residual and cost describe the ACCEPTED point that was written out, never a rejected trial point.  One documented
 * exception: a nested start of the lane kernel without confirm_full_pass may take the step after a lane's first as it
 * is - a Gauss-Newton step of at most 1e-5 mm whose PREDICTED successor is below a thousandth of step_tol - without
 * evaluating the point it lands on; the two fields are then those of the point that step started from (at most
 * max_i |J_i|_1 * last_step from the rows of the returned state; ~1e-8 mm in practice), last_step is that step.
 * Non-finite input (a NaN or infinite target, a NaN or infinite entry of the geometry's tables): the problem is never
 * accepted - bit0 stays clear.  bit2 is set as soon as a non-finite cost is met at a point the problem stands on: at its
 * first evaluation, in the shared first step's table entry when that step is NaN, or at the re-evaluation of the accepted
 * point after a non-finite trial point was rejected (an infinite target under the shared first step takes that way: a
 * launch with max_iter = 1 ends before it, with neither bit0 nor bit2); likewise when a computed correction is NaN.
 * cost is then that non-finite value and the positions are the state the problem stood on.  max_residual is formed
 * with NaN-dropping maxima: in such a record it may be finite and small, and says nothing.  Other problems of the
 * launch are not affected, and a chain restarts from the design state at the next problem. */
typedef struct okx_info {
  double max_residual;    /* max |r_i| at the returned state, reference row definitions    */
  double cost;            /* 0.5 * sum r_i^2 at the returned state                         */
  double last_step;       /* max|dx| of the last accepted step                             */
  int32_t iterations;     /* LM iterations used                                            */
  int32_t nfev;           /* residual evaluations (SolverInfo.nfev analogue)               */
  int32_t flags;          /* bit0 converged, bit1 max_residual > residual_tolerance,
                             bit2 damping failure / non-finite, bit3 ill-conditioned: in the last
                             factorisation (smallest pivot - damping) / largest pivot fell below
                             OKX_ILL_CONDITIONED_PIVOT_RATIO, i.e. cond(J) above ~1e6: a singular
                             configuration, typically a compromise point just beyond kinematic
                             lock-out whose residual is still inside residual_tolerance.  The
                             minimiser is only defined to ~cond(J) * eps * |x| there: advisory.
                             (quad kernel and the one-problem-per-wavefront interpreter).  Pair-mode kernels
                             test the halves' pivots and the stiffness of the mode their joining row ties
                             together.  The generated kernels test, beside the pivots (lower bounds of the
                             smallest eigenvalue), the Rayleigh quotient of the last step in J^T J + lambda I less
                             lambda (an upper bound, close where J is singular): a singular direction spread
                             over several pivots leaves every one of them well above the damping.  A solve that
                             ends on the ftol test while missing its rows by more than 1 % of
                             residual_tolerance (a compromise point) sets it as well.                       */
  int32_t reserved;
} okx_info;

#define OKX_INFO_CONVERGED 1
#define OKX_INFO_RESIDUAL_EXCEEDED 2
#define OKX_INFO_FAILED 4
#define OKX_INFO_ILL_CONDITIONED 8
#define OKX_ILL_CONDITIONED_PIVOT_RATIO 1e-12 /* (min pivot - lambda) / max pivot of the LDL^T of J^T J + lambda I */

int32_t okx_abi_version(void);
const char* okx_last_error(void);
void okx_default_opts(okx_solve_opts* opts);

/* Number of visible HIP devices (0 when there is no GPU); never fails. */
int32_t okx_device_count(void);

/*
 * Replaces ResidualComputer.__init__/build_jac_plan (solver.py:187-214, :281-500):
 * validates the program, uploads it to the current HIP device and precomputes the
 * sparsity plan.  Returns OKX_ERR_UNDERDETERMINED like validate_least_squares_dimensions
 * (solver.py:99-121).
 */
int32_t okx_program_create(const okx_program_desc* desc, okx_program** out);
void okx_program_destroy(okx_program* prog);

/*
 * Replaces solve_suspension_sweep (solver.py:654-776) for a batch of B sweep-step
 * problems.  d_targets holds the ABSOLUTE target scalars (convert_targets_to_absolute,
 * solver.py:584-627, is host work).  For a perturbed-geometry ensemble pass G geometries:
 * d_geom_pos [G][P][3] design positions and d_geom_row_param [G][Mc][8] row parameters
 * (see okx_rebind_design); pass NULL for both to use the program's own geometry.
 * Outputs: d_out_pos [B][n_out][3] solved positions of the output points
 * (SuspensionState.positions, state.py:119-126) and d_info [B].
 */
int32_t okx_solve_batch(okx_program* prog, const okx_solve_opts* opts, int64_t n_problems,
                        const double* d_targets,          /* [B][T] */
                        const double* d_geom_pos,         /* [G][P][3] or NULL */
                        const double* d_geom_row_param,   /* [G][Mc][8] or NULL */
                        double* d_out_pos,                /* [B][n_out][3] */
                        okx_info* d_info,                 /* [B] */
                        void* stream);

/*
 * Which kernel family and chain length okx_solve_batch (evaluated != 0: okx_solve_evaluated_batch) would use for a launch
 * of n_problems with these options, with (geometry_tables != 0) or without per-geometry tables; nothing is launched.
 * out2[0]: the okx_solve_opts.kernel value that forces the same family (1 interpreter, 2 packed interpreter, 3 quad, 4 lane);
 * out2[1]: the chain length the launch resolves chain / chain_len to (-1: the lane kernel's nested start mode, which sizes
 * itself from steps_per_geometry alone).  The selection depends on the problem count: a caller that cuts one batch into
 * several launches and needs the BITS of the single launch (the multi-GPU ensemble's chunks, dist.py) asks once for the
 * whole batch and passes the answer to every piece.  No reference counterpart (the reference has one code path).
 */
int32_t okx_plan_launch(okx_program* prog, const okx_solve_opts* opts, int64_t n_problems, int32_t geometry_tables,
                        int32_t evaluated, int32_t* out2);

/*
 * Replaces ResidualComputer.compute / compute_jacobian (solver.py:226-275, :502-581)
 * for B free-coordinate vectors: d_x [B][n] -> d_r [B][m], d_jac [B][m][n] (row-major,
 * dense).  d_jac may be NULL.  Used by the parity tests (rung R1).
 */
int32_t okx_eval_batch(okx_program* prog, int64_t n_problems,
                       const double* d_x,                 /* [B][n] */
                       const double* d_targets,           /* [B][T] */
                       double* d_r,                       /* [B][m] */
                       double* d_jac,                     /* [B][m][n] or NULL */
                       void* stream);

/*
 * Per-geometry problem emission on device (reference: topology constraints() computing
 * design lengths/angles/volumes from the initial state, e.g. double_wishbone.py:259-308,
 * track_rod.py:60-97, attachments.py:23-121).  d_hardpoints [G][P][3] holds design
 * positions of the fixed and free points (derived entries are ignored and recomputed).
 * Writes d_geom_pos [G][P][3] (derived points filled in) and d_geom_row_param [G][Mc][8]
 * with every row's design-state target recomputed (distance L, angle alpha, triple
 * product V and scale=|V|, point-on-line / line-pin anchor = the point's design position);
 * rows whose parameters are authored constants (fixed axis, planes) are copied through.
 *
 * Derived-op parameters are PROGRAM CONSTANTS: every geometry's derived points are recomputed
 * with the program's own dop_param - the ALONG offset (wheel offset, half wheel width, the
 * MacPherson strut clamp's distance from the lower ball joint) and the contact-patch radius.
 * The reference reads the clamp offset off the AUTHORED clamp of each geometry
 * (macpherson.py:199-204, :302-323: the clamp projected onto the strut axis); here an authored
 * clamp entry in d_hardpoints is ignored like every other derived entry, and the clamp is
 * placed at LBJ + normalize(STRUT_TOP - LBJ) * d0 with the program's d0.  A table whose
 * clamps keep the distance d0 along their own perturbed axis describes the same mechanisms as
 * the reference builds; one that moves the clamp along the axis does not (the solve kernels
 * read the same constant), and DeviceProgram.rebind(strict=True) refuses it.  Both are pinned
 * against the reference on every topology by tests/test_gpu_rebind_topologies.py.
 */
int32_t okx_rebind_design(okx_program* prog, int64_t n_geometries,
                          const double* d_hardpoints,     /* [G][P][3] */
                          double* d_geom_pos,             /* [G][P][3] */
                          double* d_geom_row_param,       /* [G][Mc][8] */
                          void* stream);

/* Health of one tangent solve, the device analogue of TangentSolveInfo (sensitivity.py:44-55):
 * the pivots of the LDL^T of J^T J stand in for the singular values of J: they lie inside
 * [s_min^2, s_max^2], so sqrt(max_pivot / min_pivot) is a lower bound of J's condition number
 * and a non-positive or vanishing pivot signals rank deficiency. */
typedef struct okx_tangent_info {
  double min_pivot;       /* smallest pivot of the LDL^T of J^T J                          */
  double max_pivot;       /* largest pivot                                                 */
  int32_t flags;          /* bit0 factorisation succeeded, bit1 rank deficient
                             (min_pivot <= n * eps * max_pivot or a non-positive pivot)    */
  int32_t reserved;
} okx_tangent_info;

#define OKX_TANGENT_OK 1
#define OKX_TANGENT_RANK_DEFICIENT 2

/*
 * Replaces compute_state_tangents / compute_sweep_tangents (sensitivity.py:57-143,
 * sweep.py:113-141) for B solved states: with J the analytical Jacobian at the state
 * (constraint rows + target rows; the pinned line rows play the role of the reference's
 * _degenerate_constraint_pins, sensitivity.py:146-174), solves J q_t = e_t in the
 * least-squares sense for every target row t (q_t = (J^T J)^-1 J^T e_t) and propagates the
 * free-point velocities to every derived point in forward mode.  d_pos [B][n_out][3] are
 * solved positions as written by okx_solve_batch (every free point must be an output
 * point); d_tangents [B][T][n_out][3] receives d(point)/d(target t); fixed points get 0.
 * Geometry tables as in okx_solve_batch.  Programs with a quad kernel use its generated
 * tangent kernel (16 states per wavefront); all others the generic interpreter form (one
 * wavefront per state).
 */
int32_t okx_tangent_batch(okx_program* prog, int64_t n_problems, int64_t steps_per_geometry,
                          const double* d_pos,            /* [B][n_out][3] */
                          const double* d_geom_pos,       /* [G][P][3] or NULL */
                          const double* d_geom_row_param, /* [G][Mc][8] or NULL */
                          double* d_tangents,             /* [B][T][n_out][3] */
                          okx_tangent_info* d_tinfo,      /* [B] */
                          void* stream);

/*
 * Corner state metrics: pure functions of solved points, evaluated for B
 * states in one streaming launch.  Roles are indices into the OUTPUT point list of the
 * program the positions come from (Suspension.wheel_axis_points(), steering_axis_points(),
 * suspensions/corner/base.py role hooks).
 */
typedef struct okx_corner_roles {
  int32_t wheel_center, contact_patch;   /* PointID.WHEEL_CENTER, CONTACT_PATCH_CENTER        */
  int32_t axle_inboard, axle_outboard;   /* wheel_axis_points()                               */
  int32_t steer_lower, steer_upper;      /* steering_axis_points() (lower, upper pivot)       */
  /* Instant axis of the upright (compute_instant_axis): OKX_IA_TWO_PLANES = upper and lower wishbone
   * planes, points (upper front, upper rear, upper outboard, lower front, lower rear, lower outboard)
   * (corner/double_wishbone.py:376-403); OKX_IA_PLANE_AND_STRUT = lower-arm plane and the plane through
   * the strut top normal to the strut, points (arm front, arm rear, ball joint, strut top, -, -)
   * (corner/macpherson.py:325-355); OKX_IA_NONE: the instant-centre family reads NaN. */
  int32_t instant_axis_kind;
  int32_t instant_axis_point[6];
  int32_t damper_top, damper_bottom;     /* damper_points() or -1, -1 (travel.py:48-62)        */
  int32_t rack_attachment;               /* rack_attachment_point() or -1 (axle_metrics.py:60-70) */
  int32_t axle_position, driven_axle;    /* OKX_AXLE_UNSET / _FRONT / _REAR (schema/config.py:79-80,140) */
  double side_sign;                      /* +1 left, -1 right (Side.lateral_sign)             */
  double design_wheel_center_z;          /* travel reference (metrics/context.py:42-45)       */
  double design_contact_patch_z;         /* ride-height reference (axle_metrics.py:33-37)     */
  double design_rack_y;                  /* rack reference (axle_metrics.py:66-69)            */
  double wheelbase, cg_z;                /* config.wheelbase, config.cg_position.z            */
  double front_brake_bias;               /* config.front_brake_bias, NaN when unset           */
} okx_corner_roles;

enum { OKX_IA_NONE = 0, OKX_IA_TWO_PLANES = 1, OKX_IA_PLANE_AND_STRUT = 2 };
enum { OKX_AXLE_UNSET = 0, OKX_AXLE_FRONT = 1, OKX_AXLE_REAR = 2 };

/* The reference's corner metric catalog (metrics/catalog.py:46-146).  A metric the reference
 * reports as None (undefined geometry, unset configuration) reads NaN. */
enum {
  OKX_METRIC_CAMBER = 0,           /* deg, metrics/angles.py:22-50            */
  OKX_METRIC_CASTER = 1,           /* deg, angles.py:53-71                    */
  OKX_METRIC_KPI = 2,              /* deg, angles.py:74-94                    */
  OKX_METRIC_ROADWHEEL_ANGLE = 3,  /* deg (= toe), angles.py:97-132           */
  OKX_METRIC_WHEEL_TRAVEL = 4,     /* mm, travel.py:19-32                     */
  OKX_METRIC_HALF_TRACK = 5,       /* mm, travel.py:35-45                     */
  OKX_METRIC_SCRUB_RADIUS = 6,     /* mm, steering_geometry.py:22-54          */
  OKX_METRIC_MECHANICAL_TRAIL = 7, /* mm, steering_geometry.py:57-76          */
  OKX_METRIC_SVIC_X = 8,           /* mm, side-view instant centre, catalog.py:95-100 */
  OKX_METRIC_SVIC_Z = 9,
  OKX_METRIC_SVSA_LENGTH = 10,     /* mm, swing_arms.py:45-59                 */
  OKX_METRIC_FVIC_Y = 11,          /* mm, front-view instant centre, catalog.py:104-109 */
  OKX_METRIC_FVIC_Z = 12,
  OKX_METRIC_FVSA_LENGTH = 13,     /* mm, signed, swing_arms.py:62-88         */
  OKX_METRIC_DAMPER_LENGTH = 14,   /* mm, travel.py:48-62                     */
  OKX_METRIC_SVSA_ANGLE = 15,      /* deg, anti_geometry.py:32-58             */
  OKX_METRIC_ANTI_DIVE = 16,       /* %, anti_geometry.py:75-116              */
  OKX_METRIC_ANTI_LIFT = 17,       /* %, anti_geometry.py:119-160             */
  OKX_METRIC_ANTI_SQUAT = 18,      /* %, anti_geometry.py:163-206             */
  OKX_METRIC_COUNT = 19
};

/*
 * Replaces compute_metrics_for_state's catalog entries (metrics/main.py:150-185, catalog.py) and,
 * given the tangents of okx_tangent_batch, the raw material of the derivative columns
 * (metrics/derivatives.py): d_dmetrics[b][t][m] = d metric_m / d target_t,
 * e.g. deriv_camber_wrt_hub_z = d_dmetrics[.][bump target][OKX_METRIC_CAMBER],
 * deriv_damper_length_wrt_hub_z likewise, and
 * deriv_wheel_center_x_wrt_hub_z = d_tangents[.][bump target][wheel_center][0].
 * (The instant-centre family has no derivative column in the reference; its entries are the
 * forward-mode derivatives of the same formulas.)  d_tangents / d_dmetrics may both be NULL.
 */
int32_t okx_corner_metrics_batch(const okx_corner_roles* roles, int64_t n_states, int32_t n_out, int32_t n_targets,
                                 const double* d_pos,       /* [B][n_out][3] */
                                 const double* d_tangents,  /* [B][T][n_out][3] or NULL */
                                 double* d_metrics,         /* [B][OKX_METRIC_COUNT] */
                                 double* d_dmetrics,        /* [B][T][OKX_METRIC_COUNT] or NULL */
                                 void* stream);

/* Axle-scope state metrics of a solved two-corner axle (metrics/axle_metrics.py:21-95). */
enum {
  OKX_AXLE_METRIC_HEAVE = 0,               /* mm, mean wheel-centre rise                        */
  OKX_AXLE_METRIC_ROLL = 1,                /* deg, atan2(left - right rise, track)              */
  OKX_AXLE_METRIC_RIDE_HEIGHT_CHANGE = 2,  /* mm, -mean contact-patch rise                      */
  OKX_AXLE_METRIC_TRACK = 3,               /* mm, |CP_y left - CP_y right|                      */
  OKX_AXLE_METRIC_ROLL_CENTER_Y = 4,       /* mm, the two contact-patch -> FVIC lines meet here */
  OKX_AXLE_METRIC_ROLL_CENTER_Z = 5,
  OKX_AXLE_METRIC_RACK_DISPLACEMENT = 6,   /* mm, left rack pickup y - design (NaN: no rack)    */
  OKX_AXLE_METRIC_COUNT = 7
};

/* left / right: roles of the two corners as indices into the AXLE program's output points. */
int32_t okx_axle_metrics_batch(const okx_corner_roles* left, const okx_corner_roles* right, int64_t n_states,
                               int32_t n_out,
                               const double* d_pos,  /* [B][n_out][3] */
                               double* d_metrics,    /* [B][OKX_AXLE_METRIC_COUNT] */
                               void* stream);

/*
 * The EVALUATED solve (SURVEY.md section 8f.1-2 as ONE launch).  Replaces solve_evaluated_sweep / evaluate_solved_sweep
 * (core/sweep.py:217-270: solve -> compute_sweep_tangents -> compute_sweep_metrics; its sweep diagnostics are okx_diagnose_sweeps_batch) for a batch:
 * the generated solve kernels end every problem with an epilogue that, at the converged state still in registers,
 * evaluates the Jacobian once more, factors the undamped J^T J, substitutes once per target for the solution-manifold
 * tangent (sensitivity.py:57-143) and evaluates the corner metric catalog and its derivatives along every tangent
 * (metrics/catalog.py, metrics/derivatives.py) - no position records are re-read, no tangent tensor is materialised
 * unless asked for.
 *
 * d_eval [B][1 + T][OKX_EVAL_COLUMNS] receives, per problem,
 *   row 0      : columns 0 .. OKX_METRIC_COUNT-1 the metric values (NaN where the reference reports None),
 *                OKX_EVAL_MIN_PIVOT / _MAX_PIVOT / _TANGENT_FLAGS the health of the tangent solve (okx_tangent_info's
 *                fields; the flags as a double), the rest 0;
 *   row 1 + t  : columns 0 .. OKX_METRIC_COUNT-1 d metric / d target t, OKX_EVAL_RATE_WHEEL_CENTER_X .. _Z the wheel centre's
 *                velocity along that tangent, OKX_EVAL_RATE_RACK_Y the rack pickup's lateral velocity (NaN: no rack) - the
 *                driver rates the reference's deriv_<response>_wrt_<driver> columns divide by (derivatives.py:265-320).
 * The role POINTS of `roles` are compiled into the program's evaluated kernels (okx_program_enable_evaluation: generated
 * and compiled like the solve kernels, kept in the same cache; a miss compiles in place, 10 ... 60 s - okx_precompile_evaluation
 * fills the cache ahead of time); its numbers (side sign, vehicle data, design references) are kernel arguments and may
 * change from call to call through okx_program_enable_evaluation at no cost.  With geometry tables the design references
 * (wheel travel, ride height, rack displacement) are each geometry's own design state, taken from d_geom_pos.
 * Programs with a single-mode quad kernel (corners: up to 9 free points, every free point an output point, at least one
 * target); okx_solve_opts.output still says what goes to d_out_pos (OKX_OUTPUT_NONE: nothing - metrics only).
 */
#define OKX_EVAL_COLUMNS 24
enum {
  OKX_EVAL_MIN_PIVOT = 19, OKX_EVAL_MAX_PIVOT = 20, OKX_EVAL_TANGENT_FLAGS = 21,                 /* row 0 */
  OKX_EVAL_RATE_WHEEL_CENTER_X = 19, OKX_EVAL_RATE_WHEEL_CENTER_Y = 20, OKX_EVAL_RATE_WHEEL_CENTER_Z = 21,
  OKX_EVAL_RATE_RACK_Y = 22                                                                      /* rows 1 + t */
};
int32_t okx_program_enable_evaluation(okx_program* prog, const okx_corner_roles* roles);
/* bit0: the program has evaluated kernels for the roles last enabled; bit1: a lane form exists as well. */
int32_t okx_program_evaluation(const okx_program* prog);
const char* okx_program_evaluation_note(const okx_program* prog);
/* okx_solve_batch with the epilogue: d_tangents [B][T][n_out][3] and d_eval may each be NULL (not both). */
int32_t okx_solve_evaluated_batch(okx_program* prog, const okx_solve_opts* opts, int64_t n_problems,
                                  const double* d_targets, const double* d_geom_pos, const double* d_geom_row_param,
                                  double* d_out_pos, okx_info* d_info, double* d_tangents, double* d_eval, void* stream);
/* The same epilogue on given solved states d_pos [B][n_out][3] (evaluate_solved_sweep, core/sweep.py:217-245). */
int32_t okx_evaluate_batch(okx_program* prog, int64_t n_problems, int64_t steps_per_geometry, const double* d_pos,
                           const double* d_geom_pos, const double* d_geom_row_param, double* d_tangents, double* d_eval,
                           void* stream);
/* Generate + compile a program's evaluated kernels for `roles` into the on-disk cache (no device needed). */
int32_t okx_precompile_evaluation(const okx_program_desc* desc, const okx_corner_roles* roles);

/*
 * Signed rotation of output points about fixed axes from their design positions, in degrees
 * (metrics/kernels.py:58-76 rotation_about_fixed_axis_deg, vector_utils/geometric.py:31-52): the
 * topology-specific state metrics rocker_angle / torsion_bar_twist (corner/mechanisms.py:378-407,611-623:
 * PUSHROD_INBOARD about the rocker axis, times Side.lateral_sign) and arb_arm_angle / arb_twist
 * (axle/mechanisms.py:402-430: DROPLINK_U_BAR of each side about the U-bar axis; twist = left - right),
 * and with tangents their derivative columns (deriv_rocker_angle_wrt_hub_z, deriv_arb_twist_wrt_hub_z_*).
 * A point on its axis (either perpendicular below 1e-6) reads NaN where the reference raises.
 */
#define OKX_MAX_ROTATIONS 8
/* What a role measures (`kind`).  0 is the rotation described above; the others are the state metrics of an axle's
 * shared hardware that are not rotations of one point about a fixed axis (axle/mechanisms.py:718-815, :903-944),
 * evaluated by the same kernel, with the same derivative columns:
 *   1  rotation about the fixed axis of the MIDPOINT of output points `point` and `point_b` from `design` (a rigid T-bar's
 *      t_bar_heave_angle: crossbar midpoint about the pivot's lateral axis, mechanisms.py:763-798), degrees x scale;
 *   2  twist of the segment `point` - `point_b` about the MOVING stem from `axis_point` (the pivot) to the segment's
 *      midpoint, measured from `axis_dir` (the lateral direction) and taken relative to `design[0]` (the design twist in
 *      degrees): a T-bar's arb_twist (mechanisms.py:800-815), degrees;
 *   3  distance between `point` and `point_b` (a rocker-to-rocker heave link's heave_link_length, mechanisms.py:934-944), mm;
 *   4  coordinate of the midpoint of `point` and `point_b` along `axis_dir` from `axis_point` (t_bar_center_x and its
 *      rate, mechanisms.py:718-761), mm. */
#define OKX_ROLE_AXIS_ROTATION 0
#define OKX_ROLE_MIDPOINT_ROTATION 1
#define OKX_ROLE_STEM_TWIST 2
#define OKX_ROLE_DISTANCE 3
#define OKX_ROLE_MIDPOINT_COORDINATE 4
typedef struct okx_rotation_role {
  int32_t point;         /* output-point index of the moving pickup   */
  int32_t point_b;       /* second output point (kinds 1-4; unused by kind 0) */
  double design[3];      /* its design position (kind 2: design[0] = the design twist in degrees) */
  double axis_point[3];  /* a point on the fixed axis                  */
  double axis_dir[3];    /* unit direction of the axis                 */
  double scale;          /* Side.lateral_sign, or 1                    */
  int32_t kind;          /* OKX_ROLE_* */
  int32_t reserved;
} okx_rotation_role;

int32_t okx_axis_rotation_batch(const okx_rotation_role* roles, int32_t n_roles, int64_t n_states, int32_t n_out,
                                int32_t n_targets,
                                const double* d_pos,       /* [B][n_out][3] */
                                const double* d_tangents,  /* [B][T][n_out][3] or NULL */
                                double* d_angles,          /* [B][n_roles] */
                                double* d_dangles,         /* [B][T][n_roles] or NULL */
                                void* stream);

/*
 * The evaluated solve of a COMPOSED AXLE (two identical corners joined by rack / anti-roll bar / heave-link rows; the
 * generated kernels' pair mode): okx_solve_evaluated_batch / okx_evaluate_batch on a program enabled with
 * okx_program_enable_axle_evaluation end every problem with ONE epilogue for the whole axle - one undamped refactorisation
 * through the halves' factors and the joining rows' Woodbury system, one substitution per target (sensitivity.py:57-174,
 * the partner half's share exchanged inside the wavefront), derived-point velocities, then
 *   - BOTH corners' metric catalogs with their derivative along every target's tangent (metrics/main.py:63-185 per side),
 *   - the axle-scope metrics (metrics/axle_metrics.py:21-95) and their derivatives,
 *   - up to OKX_MAX_ROTATIONS roles of okx_rotation_role's kinds (rocker angles, U-bar arm angles, a T-bar's heave angle,
 *     twist and centre travel, a heave link's length: corner/mechanisms.py:378-407, axle/mechanisms.py:402-430,718-815,903-944)
 * - what solve -> okx_tangent_batch -> okx_corner_metrics_batch x 2 -> okx_axle_metrics_batch -> okx_axis_rotation_batch
 * compute in six launches.  Reference: core/sweep.py:113-173,217-270 for an AxleSuspension.
 * d_eval is [B][1 + T][OKX_EVAL_AXLE_COLUMNS]; T = the PROGRAM's targets.  Per row:
 *   columns OKX_EVAL_AXLE_LEFT  + 0 .. 23 : the left corner's block in the corner layout above (row 0: metric values, the
 *                                            tangent solve's pivots and flags; row 1 + t: derivatives, wheel-centre and rack rates),
 *   columns OKX_EVAL_AXLE_RIGHT + 0 .. 23 : the right corner's (its pivot columns are 0),
 *   columns OKX_EVAL_AXLE_METRICS + OKX_AXLE_METRIC_* : the axle-scope metrics (row 0) / their derivatives (row 1 + t),
 *   columns OKX_EVAL_AXLE_ROLES + k       : role k's value (row 0) / its rate along target t's tangent (row 1 + t).
 * The role POINTS (both corners' and the roles' `point` / `point_b`, and the roles' kinds) are compiled into the module;
 * every number (side signs, design references, vehicle data, the roles' axes, design positions and scales) is a kernel
 * argument.  The two corners must use the same instant-axis construction and both or neither carry damper / rack roles.
 */
#define OKX_EVAL_AXLE_COLUMNS 64
enum { OKX_EVAL_AXLE_LEFT = 0, OKX_EVAL_AXLE_RIGHT = 24, OKX_EVAL_AXLE_METRICS = 48, OKX_EVAL_AXLE_ROLES = 56 };
typedef struct okx_axle_roles {
  okx_corner_roles left, right;  /* indices into the AXLE program's output points */
  int32_t n_roles;               /* 0 .. OKX_MAX_ROTATIONS */
  int32_t reserved;
  okx_rotation_role roles[OKX_MAX_ROTATIONS];
} okx_axle_roles;
int32_t okx_program_enable_axle_evaluation(okx_program* prog, const okx_axle_roles* roles);
int32_t okx_precompile_axle_evaluation(const okx_program_desc* desc, const okx_axle_roles* roles);
/* Columns per row of d_eval for the evaluation last enabled: OKX_EVAL_COLUMNS (corner), OKX_EVAL_AXLE_COLUMNS (axle), 0 (none). */
int32_t okx_program_eval_columns(const okx_program* prog);

/*
 * Output positions from free-point coordinates: fixed points come from the program's design state (or the
 * per-geometry table of okx_rebind_design), derived points are re-evaluated (DerivedPointsManager.update,
 * points/derived/manager.py).  The receiving side of a multi-GPU exchange that ships the 3 n_free free
 * coordinates of each solve instead of its 3 n_out output coordinates; also turns stored free vectors
 * (SuspensionState.get_free_array) back into full states.
 */
int32_t okx_expand_positions_batch(okx_program* prog, int64_t n_problems, int64_t steps_per_geometry,
                                   const double* d_free,      /* [B][n_free][3], free_point order */
                                   const double* d_geom_pos,  /* [G][n_points][3] or NULL */
                                   double* d_out_pos,         /* [B][n_out][3] */
                                   void* stream);

/*
 * Chain-head predictor.  The reference warm-starts step k from step k-1 (solver.py:774) and starts a
 * sweep at the design state; a batch that fills the chip solves every step as an independent cold
 * start instead.  okx_program_fit_predictor solves the program once at the Chebyshev
 * nodes of a target box [lo, hi] (host arrays of n_targets absolute target values; lo[t] == hi[t]
 * holds target t), i.e. (degree + 1)^d cold solves for d varying targets in one synchronous launch,
 * and keeps the Chebyshev coefficients of every free coordinate up to total degree `degree` (1..12;
 * <= 0: 7).  Launches with opts.predictor != 0 on the program's own geometry start every chain head at that
 * polynomial (targets clamped to the box).  The LM iteration, its stopping rules and the results (to
 * step_tol) are unchanged; only the number of passes drops.  Needs the program's quad kernel and every
 * free point among the output points.  Fitting again replaces the model.
 */
int32_t okx_program_fit_predictor(okx_program* prog, const double* lo, const double* hi, int32_t degree, void* stream);
int32_t okx_program_has_predictor(const okx_program* prog);

/*
 * Camber-shim setup solve: the pose a double-wishbone corner takes when the split
 * upright's shim stack is changed from its design to its setup thickness, for n_geometries
 * geometries at once.  Replaces solve_camber_shim_assembly (suspensions/config/shims.py:284-501: 7 or 8
 * variables, 10 or 11 residuals, scipy MINPACK `lm`) and DoubleWishboneSuspension.apply_camber_shim
 * (corner/double_wishbone.py:501-570): the upper ball joint moves on the upper wishbone's arc, the
 * upright's attachments rotate about the lower ball joint, an upright-mounted pushrod turns the
 * rocker group.  Indices are rows of the point table the positions are given in (the program's
 * point list: okx_program_desc.design_pos).  The table is rewritten in place and can go straight
 * into okx_rebind_design.
 */
#define OKX_SHIM_MAX_POINTS 8
#define OKX_SHIM_PARAMS 11 /* per geometry: face point a (3), face point b (3), face normal (3), design, setup thickness
                              (CamberShimConfig, schema/config.py:52-70) */
typedef struct okx_shim_roles {
  int32_t upper_outboard, lower_outboard;            /* UPPER_/LOWER_WISHBONE_OUTBOARD (ball joints)      */
  int32_t upper_inboard_front, upper_inboard_rear;   /* upper wishbone axis (shims.py:386-390)            */
  int32_t heading_inboard, heading_outboard;         /* installed track rod / toe link (shims.py:399-403) */
  int32_t n_upright_points;                          /* upright_attachment_points() (double_wishbone.py:572-581) */
  int32_t upright_point[OKX_SHIM_MAX_POINTS];
  int32_t rocker;                                    /* 1: upright-mounted pushrod (CamberShimRockerCoupling, shims.py:49-56) */
  int32_t rocker_axis_a, rocker_axis_b, pushrod_inboard, pushrod_outboard;
  int32_t n_rocker_points;                           /* rocker group (mechanisms.py:247-265)              */
  int32_t rocker_point[OKX_SHIM_MAX_POINTS];
} okx_shim_roles;

typedef struct okx_shim_info {
  double residual_norm;       /* CamberShimAssemblySolution.constraint_residual_norm             */
  double max_residual;
  double upright_angle_rad;   /* upright_body_rot_angle_rad                                      */
  double rocker_angle_rad;
  double wishbone_angle_rad;
  int32_t converged;          /* max residual <= SOLVE_ACCEPT_RESIDUAL (shims.py:456-462)        */
  int32_t iterations;
} okx_shim_info;

int32_t okx_camber_shim_batch(const okx_shim_roles* roles, int64_t n_geometries, int32_t n_points,
                              double* d_points,        /* [G][n_points][3] in: authored, out: setup */
                              const double* d_shim,    /* [G][OKX_SHIM_PARAMS] */
                              okx_shim_info* d_info,   /* [G] or NULL */
                              void* stream);

/*
 * Runtime specialisation.  okx_program_create also GENERATES a HIP kernel for the program at
 * hand (straight-line residual / Jacobian / normal-equation / LDL^T code, four lanes per
 * problem), compiles it with hiprtc and loads it; the reference does the analogous thing
 * offline for its Jacobian rows (tools/generate_jacobians.py -> core/jacobians.py) and
 * interprets the rest per call (solver.py:226-275, :502-581).  Code objects are cached under
 * <directory of libokx.so>/_kcache (override: OKX_KERNEL_CACHE), keyed by the generated source.
 * Programs the generator has no code path for (more than 9 free points and no pair structure, unsupported row or
 * derived-point types) keep the generic interpreter kernels; nothing else changes for them.
 */

/* "quad" when the specialised kernel of this program is loaded, "wave" when the generic
 * interpreter kernels are in charge; okx_program_kernel_note() then says why (static strings
 * owned by the program). */
const char* okx_program_kernel(const okx_program* prog);
const char* okx_program_kernel_note(const okx_program* prog);
/* 1 when chain heads of the program's own geometry take their first Levenberg-Marquardt step from the shared first-step
 * table (okx_solve_opts.shared_first_step): okx_info.nfev of such a head does not count the design-state evaluation,
 * which was made once for all of them (the drop-in's SolverInfo.nfev adds it back, solver.py:766-771). */
int32_t okx_program_shares_first_step(const okx_program* prog);
/* 1 when launches of INDEPENDENT solves (chain length 1) on the program's own geometry with the shared first step run the
 * quad kernel's cold body `okx_quad_cold_u` (no chain history, no fitted model, no trace: tables staged through LDS, the
 * passes of an all-accepted solve under one exec mask, anything else redone through the general loop - same answers, bit
 * for bit, as `okx_quad_solve_u`).  What bench.py names as the dominant kernel of the headline launch. */
int32_t okx_program_has_cold_body(const okx_program* prog);
/* Tiered start.  okx_program_create loads a program's generated kernels when the kernel cache holds them (what
 * okx_precompile and __graft_entry__.build() are for).  When it does not, the call still returns at once: a host thread
 * runs the compiler (10 ... 80 s per module; it owns its inputs, so destroying the program does not wait for it) while the
 * interpreter kernels solve - same answers to 1e-9 mm, 20 ... 100 x slower - and the first launching call after the job
 * has finished switches the program over: it loads the job's code objects from memory (a few milliseconds on the calling
 * thread; never the compiler, never a synchronise of the legacy stream) while holding the program's kernel state
 * exclusively - launches of the same program from other threads wait for it, launches in progress finish first.  A call
 * whose stream is recording a HIP graph never switches over (module loads are illegal in a capture): the interpreter
 * serves it and a later call does.  The switch-over has two stages: the quad module is attached as soon as IT is compiled
 * (it serves every batch size), the lane module when the whole job is done.  okx_program_ready returns 1 when nothing is
 * pending any more and 0 while the job
 * runs; wait != 0 blocks until it has finished and switches over before returning (benchmarks and tests that must know
 * which kernel they time).  okx_program_kernel() / okx_program_kernel_note() report the current state. */
int32_t okx_program_ready(okx_program* prog, int32_t wait);

/* Generated source of a program's quad kernel (no device needed).  Copies at most buflen - 1
 * bytes plus a terminator into buf (buf may be NULL) and returns the size the full text
 * needs, or a negative okx_status (OKX_ERR_LIMIT: no quad kernel for this program). */
int64_t okx_quad_source(const okx_program_desc* desc, char* buf, int64_t buflen);

/* Generate + compile a program's quad kernel (and its lane kernel, when it has one) into the on-disk
 * cache (no device needed), so that a later okx_program_create only loads them. */
int32_t okx_precompile(const okx_program_desc* desc);

/*
 * The second generated kernel family: ONE LANE PER PROBLEM, 64 problems per wavefront, no cross-lane
 * operand at all (the quad kernel moves every dot product, J^T J column and pivot through DPP and idles
 * one lane in four).  About a quarter of the quad kernel's instructions per problem, but one wavefront
 * holds 64 problems and takes 25 ... 29 us whatever it holds: it pays as soon as the quad kernel (16
 * problems per wavefront, ~21 us per round) needs a second round - from okx_program_lane_threshold()
 * problems on, 16385 on an MI355X - unless an ensemble has so few steps per geometry that its lanes
 * would idle (a wave unit holds problems of ONE geometry).  Programs with at most 6 free points
 * (n <= 18) whose quad kernel is loaded have one; okx_program_lane_note() says why another has not.
 * Same algorithm, same evaluation points, same first-step tables; okx_solve_opts.kernel = 4 forces it.
 */
const char* okx_program_lane_note(const okx_program* prog);
int64_t okx_program_lane_threshold(const okx_program* prog);   /* -1: no lane kernel */
/* Which bodies auto selection uses: bit0 independent solves (chain_len 1), bit1 chains.  A body whose register
 * allocation spills more than a little stays with the quad kernel (okx_solve_opts.kernel = 4 still runs it). */
int32_t okx_program_lane_bodies(const okx_program* prog);
int64_t okx_lane_source(const okx_program_desc* desc, char* buf, int64_t buflen);

/*
 * Sweep diagnostics on device: the reference's diagnose_sweep (core/diagnostics.py:114-226 and the U-bar's
 * topology_diagnostics, axle/mechanisms.py:119-163, 432-549) for a batch of solved sweeps, one pass over the records in HBM.
 * Sweep g is states [g * steps_per_sweep, (g + 1) * steps_per_sweep) - the convention of steps_per_geometry.  Per sweep:
 *   convergence / residual   per step, from d_info (skipped when NULL): not converged; max_residual > residual_tolerance
 *   jump                     per tracked point: a step displacement above max(5 mm, 4 x the median of its strictly positive
 *                            step displacements); the median is exact (selection on the bit patterns, (a + b) / 2 at the end)
 *   chirality                per U-bar side and step: |margin| <= 1e-6 (subject bit1 set, value = margin), else the sign of the
 *                            signed volume differs from the design state's (value = the volume)
 *   transmission             per U-bar side, step and joint: |link . tangent| defined and below 0.15
 * All indices of okx_diag_roles are the PROGRAM's point indices.  The call maps them to the rows of the layout it is given
 * (OKX_OUTPUT_RECORDS [B][n_out][3] or OKX_OUTPUT_FREE [B][n_free][3], read directly); a role point that is fixed (the bar
 * axis, a rocker axis) is taken from the program's design positions or, with d_geom_pos [n_sweeps][n_points][3], from the
 * sweep's own table - as is the design state whose volume sign the chirality check compares with.  A moving point the
 * layout does not carry is OKX_ERR_INVALID.
 * Findings are appended to d_issues in no particular order; *d_issue_count ends as the number FOUND, which may exceed
 * capacity (nothing is written past it): size a second call from it.  The summaries are complete whatever the capacity.
 * Summaries and the set of issue records are bit-identical from run to run and independent of the batch they were part of.
 * Launch-only and stream-ordered (the call resets *d_issue_count on the stream itself); legal inside a stream capture.
 * Sweeps too long for one workgroup's LDS (tracked points x (steps - 1) doubles beyond ~60 KiB) stage their displacements
 * in ONE scratch buffer the program keeps, grown when a call needs more and then replaced in the order of that call's
 * stream - the rule of the solve's geometry-table scratch.  For such shapes therefore:
 *   - calls on one program are STREAM-ORDERED with each other: two of them on different streams at the same time would
 *     write each other's displacements (use one stream, or one program per stream);
 *   - run the shape once outside a stream capture first (a capture cannot grow the buffer: OKX_ERR_INVALID), and a
 *     captured graph holds the buffer it was captured with: do not run a LARGER long shape on the program while such a
 *     graph may still be replayed - growing frees the old buffer;
 *   - a call on another stream than the one that grew the buffer must be ordered after that call (an event).
 * Shapes that fit LDS (every ensemble of up to a few hundred steps) use no scratch and have none of these restrictions.
 */
enum { OKX_DIAG_CONVERGENCE = 0, OKX_DIAG_RESIDUAL = 1, OKX_DIAG_JUMP = 2, OKX_DIAG_CHIRALITY = 3, OKX_DIAG_TRANSMISSION = 4,
       OKX_DIAG_COUNT = 5 };

typedef struct okx_diag_side {
  int32_t droplink_rocker, droplink_u_bar;                                   /* moving pickups                    */
  int32_t rocker_axis_a, rocker_axis_b, pushrod_inboard, pushrod_outboard;   /* all -1: no rocker group           */
} okx_diag_side;

typedef struct okx_diag_roles {
  int32_t n_points;                   /* continuity: how many points are tracked (<= OKX_MAX_VARS / 3)             */
  int32_t point[OKX_MAX_VARS / 3];    /* ... and which, in suspension.free_points() order                          */
  int32_t n_sides;                    /* 0: no U-bar checks; 2: LEFT, RIGHT                                        */
  okx_diag_side side[2];
  int32_t bar_axis_a, bar_axis_b;     /* the U-bar axis (fixed points)                                             */
} okx_diag_roles;

typedef struct okx_diag_summary {     /* one per sweep */
  int32_t n_issues[OKX_DIAG_COUNT];
  int32_t first_step[OKX_DIAG_COUNT]; /* -1: none                                                                  */
  double worst[OKX_DIAG_COUNT];       /* over every step, issue or not: [1] largest max_residual, [2] largest step
                                         displacement (0: nothing looked at), [3] smallest |chirality margin|,
                                         [4] smallest transmission margin (+inf: nothing looked at); [0] unused      */
} okx_diag_summary;

typedef struct okx_diag_issue {       /* one per finding, the device form of DiagnosticIssue                       */
  int64_t sweep;
  int32_t step;
  int32_t category;                   /* OKX_DIAG_*                                                                */
  int32_t subject;                    /* jump: index into roles.point; chirality: side | boundary << 1;
                                         transmission: side | joint << 1 (0 bar pickup, 1 pushrod, 2 rocker pickup) */
  int32_t reserved;
  double value, threshold;
} okx_diag_issue;

int32_t okx_diagnose_sweeps_batch(okx_program* prog, const okx_diag_roles* roles, int64_t n_sweeps, int64_t steps_per_sweep,
                                  int32_t layout,               /* OKX_OUTPUT_RECORDS or OKX_OUTPUT_FREE            */
                                  const double* d_pos,
                                  const okx_info* d_info,       /* or NULL: no convergence / residual check         */
                                  const double* d_geom_pos,     /* [n_sweeps][n_points][3] or NULL                  */
                                  double residual_tolerance,
                                  okx_diag_summary* d_summary,  /* [n_sweeps]                                       */
                                  okx_diag_issue* d_issues,     /* [capacity] or NULL                               */
                                  int64_t capacity,
                                  int64_t* d_issue_count,       /* total found, may exceed capacity                 */
                                  void* stream);

/*
 * Ensemble reduction on device: per (step, column) entry of a table of metric columns, over its geometries, the raw
 * accumulators a tolerance / sensitivity study finalizes on the host (open_kinematics_amd/ensemble_stats.py).
 * d_values is [n_geometries * steps][ld] with the n_columns columns in front of every row (ld >= n_columns: the gathered
 * column table of an evaluated ensemble, or a view of its evaluation rows); geometry g is rows [g * steps, (g + 1) * steps).
 * A state counts when its status byte (d_status[row * status_stride], the low byte of okx_info.flags; NULL: every state)
 * says converged, not residual-exceeded, not failed, and its value is finite; anything else is REJECTED.
 * d_acc [steps][n_columns][OKX_ENS_FIELDS + n_factors], every field a double:
 *   OKX_ENS_COUNT, OKX_ENS_REJECTED   states that count / do not
 *   OKX_ENS_SUM, OKX_ENS_SUMSQ        sum d, sum d^2 with d = value - d_shift[step][column] over the states that count
 *   OKX_ENS_MIN, OKX_ENS_MAX          +inf / -inf when nothing counts
 *   OKX_ENS_ARGMIN, OKX_ENS_ARGMAX    geometry_offset + g of the extreme, ties to the LOWEST index, -1 when nothing counts
 *   OKX_ENS_FIELDS + p                sum f_p d over the states that count, f = d_factors [n_geometries][n_factors]
 * d_factor_acc (or NULL) [n_factors + n_factors (n_factors + 1) / 2 + 1]: sum f_p, sum f_p f_q (q <= p, lower triangle
 * row by row) and the geometry count, over EVERY geometry of the call.
 * accumulate = 1 merges into what d_acc / d_factor_acc hold (additions and comparisons only: every partial that is ever
 * merged must have been taken with the same d_shift); 0 overwrites.  n_columns = 0 computes the factor moments alone.
 * No floating-point atomics: two launches, partial accumulators per slab of geometries in d_scratch
 * (okx_ensemble_scratch_bytes of the same sizes), merged in ascending slab order.  The slab count depends on the sizes
 * alone, so the result is bit-identical from run to run and from device to device.  Launch-only, stream-ordered, legal
 * inside a stream capture; calls that share d_scratch must be stream-ordered with each other.
 */
enum { OKX_ENS_COUNT = 0, OKX_ENS_REJECTED = 1, OKX_ENS_SUM = 2, OKX_ENS_SUMSQ = 3, OKX_ENS_MIN = 4, OKX_ENS_MAX = 5,
       OKX_ENS_ARGMIN = 6, OKX_ENS_ARGMAX = 7, OKX_ENS_FIELDS = 8, OKX_ENS_MAX_FACTORS = 1024 };

int32_t okx_ensemble_reduce(int64_t n_geometries, int64_t steps, int32_t n_columns,
                            const double* d_values, int64_t ld,
                            const uint8_t* d_status, int64_t status_stride, /* or NULL                                  */
                            const double* d_factors, int32_t n_factors,     /* or NULL, 0                               */
                            const double* d_shift,                          /* [steps][n_columns]                       */
                            int64_t geometry_offset,                        /* global index of geometry 0 of this call  */
                            int32_t accumulate,
                            double* d_acc,
                            double* d_factor_acc,                           /* or NULL                                  */
                            void* d_scratch, size_t scratch_bytes, void* stream);
size_t okx_ensemble_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_factors);

/*
 * Ensemble selection on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): per (step, column)
 * entry of the same table, over the states that count by the rule of okx_ensemble_reduce, EXACT order statistics and
 * spec-limit counts - what quantiles and yield are finalized from on the host (open_kinematics_amd/ensemble_stats.py).
 * d_probs [n_probs] probabilities in [0, 1]; d_limits (or NULL) [steps][n_columns][2] = (lo, hi), -inf / +inf leaves a side
 * open.  With n the number of states that count and h = (n - 1) * p in fp64:
 *   d_order   [steps][n_columns][n_probs][2]  x[floor(h)], x[ceil(h)] of the sorted accepted values (0-based) - the bits
 *                                             of values in the table; NaN when n = 0 (or p is not in [0, 1])
 *   d_count   [steps][n_columns]              n, int64
 *   d_outside [steps][n_columns][2] or NULL   accepted values < lo, > hi (strictly), int64
 * The quantile x_lo + (h - floor(h)) (x_hi - x_lo) (NumPy's method="linear") and the yield 1 - (below + above) / n are
 * host arithmetic; p = 0 / 1 give OKX_ENS_MIN / OKX_ENS_MAX of the reduce pass bit for bit.
 *
 * A radix select on order-preserving keys: key = bits ^ (sign ? ~0 : 1 << 63) (-0.0 sorts before +0.0), and
 * okx_ensemble_select_rounds() = 64 / OKX_ENS_SELECT_BITS rounds fix OKX_ENS_SELECT_BITS key bits each, from the top.
 * Selection j = 2 q + side of an entry carries a prefix (the bits fixed so far) and the rank wanted among the values that
 * share it.  Per round: a COUNT pass adds into d_hist, int64 [steps][n_columns][2 n_probs][1 << OKX_ENS_SELECT_BITS]
 * (okx_ensemble_select_hist_len words): hist[s][k][j][b] += accepted values whose fixed bits equal selection j's prefix and
 * whose next bits are b; a DESCEND picks the bin that holds the rank, extends the prefix, subtracts what lies below and
 * re-zeroes the histogram.  Round 0 has no prefix: hist[s][k][0][:] is the histogram all selections of the entry share,
 * hist[s][k][1][0] / [1][1] count the values below lo / above hi, the rest stays zero; its descend sums n and turns the
 * probabilities into ranks.  Integer atomics only (LDS, then global) - no floating-point operation but the rank's product.
 * The histogram is ALL that depends on the data: a table that arrives in chunks counts every chunk into the same d_hist
 * before the round's descend, and ranks that hold parts of it sum their histograms (an integer all-reduce) before each
 * descends its own copy of the state - integer sums in any order, so the result is bit-identical across chunks, slabs,
 * runs, devices and ranks.  d_state (okx_ensemble_select_state_bytes) is opaque.  Launch-only, stream-ordered, legal inside
 * a stream capture: no host read-back between rounds, and begin zeroes state and histogram on the stream.
 *   okx_ensemble_select          one device, one table: begin, every round's count + descend, finish; d_scratch holds
 *                                state and histogram (okx_ensemble_select_scratch_bytes).  n_geometries = 0 is legal.
 *   okx_ensemble_select_begin    zeroes d_state and d_hist
 *   okx_ensemble_select_count    round `round` over one chunk of geometries, adds into d_hist (d_limits is read in round 0)
 *   okx_ensemble_select_descend  consumes d_hist, advances d_state, re-zeroes d_hist (d_probs is read in round 0)
 *   okx_ensemble_select_finish   writes d_order / d_count / d_outside from d_state
 * The launches cannot read d_probs / d_limits on the host: okx_ensemble_select_check validates HOST copies of them
 * (p outside [0, 1] or NaN, NaN limits, lo > hi: OKX_ERR_INVALID with okx_last_error text) before they are uploaded.
 */
#ifndef OKX_ENS_SELECT_BITS
#define OKX_ENS_SELECT_BITS 4
#endif
enum { OKX_ENS_SELECT_MAX_PROBS = 64 };

int32_t okx_ensemble_select(int64_t n_geometries, int64_t steps, int32_t n_columns,
                            const double* d_values, int64_t ld,
                            const uint8_t* d_status, int64_t status_stride, /* or NULL                                  */
                            const double* d_probs, int32_t n_probs,
                            const double* d_limits,                         /* or NULL                                  */
                            double* d_order, int64_t* d_count,
                            int64_t* d_outside,                             /* or NULL                                  */
                            void* d_scratch, size_t scratch_bytes, void* stream);
int32_t okx_ensemble_select_begin(int64_t steps, int32_t n_columns, int32_t n_probs, void* d_state, int64_t* d_hist, void* stream);
int32_t okx_ensemble_select_count(int32_t round, int64_t n_geometries, int64_t steps, int32_t n_columns,
                                  const double* d_values, int64_t ld, const uint8_t* d_status, int64_t status_stride,
                                  int32_t n_probs, const double* d_limits, const void* d_state, int64_t* d_hist, void* stream);
int32_t okx_ensemble_select_descend(int32_t round, int64_t steps, int32_t n_columns, const double* d_probs, int32_t n_probs,
                                    void* d_state, int64_t* d_hist, void* stream);
int32_t okx_ensemble_select_finish(int64_t steps, int32_t n_columns, int32_t n_probs, const void* d_state,
                                   double* d_order, int64_t* d_count, int64_t* d_outside, void* stream);
/* host only */
int32_t okx_ensemble_select_rounds(void);
int64_t okx_ensemble_select_hist_len(int64_t steps, int32_t n_columns, int32_t n_probs);
size_t okx_ensemble_select_state_bytes(int64_t steps, int32_t n_columns, int32_t n_probs);
size_t okx_ensemble_select_scratch_bytes(int64_t steps, int32_t n_columns, int32_t n_probs);
int32_t okx_ensemble_select_check(const double* probs, int32_t n_probs, const double* limits /* or NULL */, int64_t n_limits /* (lo, hi) pairs */);

/*
 * Ensemble screening on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): the JOINT verdict of
 * every geometry of the same table against d_limits [steps][n_columns][2] = (lo, hi) - what the per-entry yields of
 * okx_ensemble_select cannot give, the columns of one geometry being correlated along the sweep.  An entry is LOOKED AT
 * when at least one of its limits is finite; it COUNTS by the rule of okx_ensemble_reduce.  d_scale (or NULL: 1)
 * [steps][n_columns], finite and > 0, is the unit in which margins are compared across entries.  Per geometry of THIS call:
 *   d_flags  [n_geometries] uint8   OKX_SCREEN_OUTSIDE: a looked-at entry that counts is < lo or > hi (strictly);
 *                                   OKX_SCREEN_UNRESOLVED: a looked-at entry does not count.  0: the geometry passes.
 *   d_margin [n_geometries] double  min over the looked-at entries that count of m = min((v - lo) / scale, (hi - v) / scale),
 *                                   every operation rounded on its own (m = y < x ? y : x with x the lo side); +inf when
 *                                   nothing qualifies
 *   d_entry  [n_geometries] int32   s * n_columns + k of that minimum, the lowest on ties; -1 when nothing qualifies
 * Per ensemble, int64:
 *   d_tally  [4]                    geometries seen, passed, outside, unresolved
 *   d_blame  [steps][n_columns][2]  per OUTSIDE geometry one count at its d_entry: side 0 its value is below lo, side 1 not
 *   d_pass_index [capacity] or NULL geometry_offset + g of the passing geometries, ascending; slots at or beyond capacity
 *                                   and beyond the count are never written
 *   d_pass_count [1]                survivors found (may exceed capacity)
 * accumulate = 0 overwrites d_tally, d_blame and d_pass_count; accumulate = 1 adds into tally and blame and appends the
 * survivors after the *d_pass_count already there (read on the device, stream-ordered): chunks passed in ascending order
 * give one ascending list.  Integer atomics only, and no atomic decides a survivor's slot: the result is bit-identical
 * across chunks, launch geometries, runs, devices and ranks.  Launch-only, stream-ordered, no host read-back, legal inside
 * a stream capture; n_geometries = 0 is legal.  d_scratch: okx_ensemble_screen_scratch_bytes.  The launch cannot read
 * d_limits / d_scale on the host: okx_ensemble_screen_check validates HOST copies of them (NaN limits, lo > hi, a scale
 * that is not finite and > 0: OKX_ERR_INVALID with okx_last_error text) before they are uploaded.
 */
enum { OKX_SCREEN_OUTSIDE = 1, OKX_SCREEN_UNRESOLVED = 2 };

int32_t okx_ensemble_screen(int64_t n_geometries, int64_t steps, int32_t n_columns,
                            const double* d_values, int64_t ld,
                            const uint8_t* d_status, int64_t status_stride, /* or NULL                                  */
                            const double* d_limits,
                            const double* d_scale,                          /* or NULL                                  */
                            int64_t geometry_offset, int32_t accumulate,
                            uint8_t* d_flags, double* d_margin, int32_t* d_entry,
                            int64_t* d_tally, int64_t* d_blame,
                            int64_t* d_pass_index, int64_t capacity,        /* or NULL                                  */
                            int64_t* d_pass_count,
                            void* d_scratch, size_t scratch_bytes, void* stream);
/* host only */
size_t okx_ensemble_screen_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns);
int32_t okx_ensemble_screen_check(const double* limits, const double* scale /* or NULL */, int64_t n_entries);

/*
 * Ensemble covariance on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): how the entries of the
 * same table move TOGETHER over the geometries - what the per-entry moments, the quantiles and the per-geometry verdict do
 * not say.  d_entries: n_entries DISTINCT indices s * n_columns + k, in the order the caller wants rows and columns; NULL:
 * all steps * n_columns entries in natural order (n_entries must then be that number).  1 <= n_entries <=
 * OKX_ENS_COV_MAX_ENTRIES.  An entry COUNTS by the rule of okx_ensemble_reduce (status & 7 == 1 and a finite value).
 * COMPLETE CASES: a geometry is USED when every SELECTED entry of it counts; otherwise it is DROPPED and contributes nothing
 * (an entry that is not selected never drops a geometry).  One count therefore serves the whole matrix, the matrix is a true
 * Gram matrix (positive semidefinite up to rounding), and the used set is exactly okx_ensemble_screen's "not UNRESOLVED" for
 * the same looked-at entries.  Pairwise-complete moments are not offered.  With d = value - d_shift[entry] (d_shift
 * [steps][n_columns], indexed by the entry, finite) over the used geometries, N = n_entries:
 *   d_gram   [N][N] double  sum d_n d_m, the full square; gram[n][m] and gram[m][n] are the same bits
 *   d_sum    [N]    double  sum d_n
 *   d_counts [2]    int64   geometries used, dropped
 *   d_used   [n_geometries] uint8 or NULL: 1 where geometry g of THIS call is used
 * accumulate = 0 overwrites gram, sum and counts; accumulate = 1 adds this call after what they hold - additions only, so it
 * needs the same shift and the same entries as the calls before.  The host finishes: n = used, mean = shift + sum / n,
 * covariance = (gram - sum sum^T / n) / (n - 1) (NaN for n < 2), correlation NaN where a variance is 0.
 * Launch-only, stream-ordered, no host read-back, no allocation, legal inside a stream capture; n_geometries = 0 is legal.
 * No floating-point atomics (no atomics on device memory at all): the geometries are cut into slabs by a plan that is a
 * function of (n_geometries, steps, n_columns, n_entries) alone and never looks at the device, a slab is summed in ascending
 * geometry order, four at a time in v_mfma_f64_16x16x4_f64, and the slabs are added in ascending order per output element -
 * two runs, or two devices, give the same bits.  DIFFERENT CHUNKINGS of the same geometries agree to rounding only, as for
 * okx_ensemble_reduce: |result - exact| <= (G + 2) u sum |d_n d_m| each (exactly where every product and sum is
 * representable).  d_scratch: okx_ensemble_covariance_scratch_bytes.  The launch cannot read d_entries on the host:
 * okx_ensemble_covariance_check validates a HOST copy (an index outside [0, n_table_entries), a duplicate, a count outside
 * 1 .. OKX_ENS_COV_MAX_ENTRIES: OKX_ERR_INVALID with okx_last_error text) before it is uploaded; on the device an index out
 * of range is never dereferenced - its entry never counts, every geometry is dropped.
 */
enum { OKX_ENS_COV_MAX_ENTRIES = 2048 };

int32_t okx_ensemble_covariance(int64_t n_geometries, int64_t steps, int32_t n_columns,
                                const double* d_values, int64_t ld,
                                const uint8_t* d_status, int64_t status_stride, /* or NULL                              */
                                const int32_t* d_entries, int32_t n_entries,    /* or NULL: all, n_entries = steps * n_columns */
                                const double* d_shift,
                                int32_t accumulate,
                                double* d_gram, double* d_sum, int64_t* d_counts,
                                uint8_t* d_used,                                /* or NULL                              */
                                void* d_scratch, size_t scratch_bytes, void* stream);
/* host only */
size_t okx_ensemble_covariance_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_entries);
int32_t okx_ensemble_covariance_check(const int32_t* entries /* or NULL */, int32_t n_entries, int64_t n_table_entries);

/*
 * Ensemble curves on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): what the four passes above
 * do not look at - the shape of a column ALONG the sweep inside one geometry.  Per geometry g and column k of the same table
 * the pass writes OKX_CURVE_FIELDS doubles, d_features [n_geometries][n_columns][12], and d_count [n_geometries][n_columns]
 * int32; the features stay in HBM and are again a column table [G][K * 12] with ONE step per geometry, so
 * okx_ensemble_reduce / _select / _screen / _covariance apply to gradients and curvatures as they do to per-step values.
 * Abscissa: d_abscissa [steps], shared by every geometry, or NULL: column x_column of the table itself (every geometry is
 * fitted against its own wheel travel, say).  u = (x - origin) / scale, scale finite and > 0; the window [window_lo,
 * window_hi] is in x units and closed (-inf / +inf: open).  A step is USED for column k of geometry g when its state counts
 * by the rule of okx_ensemble_reduce (status & 7 == 1), x is finite and inside the window, and the value is finite.
 * The fit is the least-squares polynomial of degree 0 <= degree <= 3 in u over the used steps:
 *   0 .. 3   c0 .. c3 in x units about origin, c_i = a_i / scale^i: the value at the origin, the gradient there, half the
 *            curvature; degrees above `degree` are 0.0
 *   4        rms of the residuals, sqrt(sum r^2 / n)
 *   5        largest |r|: the departure from the fitted shape (linearity for degree 1)
 *   6, 7     smallest and largest used value                         (exact table bits)
 *   8, 9     the abscissa at which 6 and 7 are taken, the lowest step on ties    (exact bits)
 *   10, 11   smallest and largest used abscissa, the lowest step on ties         (exact bits)
 * With no used step all 12 fields are NaN.  With fewer than degree + 1 used steps, or a REFUSED fit, fields 0 .. 5 are NaN and
 * 6 .. 11 stand.  A fit is refused when a pivot of the Cholesky factor of the normal matrix in u (N_ij = sum u^(i + j)),
 * N_jj - sum_k L_jk^2, is not greater than 2^-40 times its diagonal entry N_jj - used abscissae that are all equal end there.
 * NaN features need no flag: every pass above treats a non-finite value as one that does not count.
 * The normal equations are solved by Cholesky in registers: |c_i scale^i - exact| is of the order cond(N) u max |y|, which
 * is why u should be of order one over the window (scale = the half width).  No atomics and no scratch; the lane plan is a
 * function of (steps, n_columns) alone and a geometry's outputs depend on its own rows only, so they are bit-identical from
 * run to run and across chunkings, devices and ranks.  Launch-only, stream-ordered, no host read-back, no allocation, legal
 * inside a stream capture; n_geometries = 0 is legal and does nothing, steps = 1 fits degree 0.  okx_ensemble_curves_check
 * validates the arguments on the host (abscissa_len: the length of the shared abscissa, < 0: a column is used) with
 * okx_last_error text; the launch runs it too.
 */
#define OKX_CURVE_FIELDS 12

int32_t okx_ensemble_curves(int64_t n_geometries, int64_t steps, int32_t n_columns,
                            const double* d_values, int64_t ld,
                            const uint8_t* d_status, int64_t status_stride, /* or NULL                                  */
                            const double* d_abscissa,                       /* [steps] or NULL                          */
                            int32_t x_column,                               /* used when d_abscissa is NULL             */
                            double origin, double scale, double window_lo, double window_hi, int32_t degree,
                            double* d_features,                             /* [n_geometries][n_columns][12]            */
                            int32_t* d_count,                               /* [n_geometries][n_columns]                */
                            void* stream);
/* host only */
int32_t okx_ensemble_curves_check(int64_t steps, int32_t n_columns, int64_t abscissa_len, int32_t x_column,
                                  double origin, double scale, double window_lo, double window_hi, int32_t degree);

/*
 * Ensemble Pareto front on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): which geometries of
 * the same table are worth keeping - those that no other geometry beats on every objective at once.  The table, the status
 * bytes and the rule by which an entry COUNTS are those of okx_ensemble_reduce (status & 7 == 1 and a finite value).
 * `entries`, `sense` and `target` are HOST arrays of n_objectives items, 1 <= n_objectives <= OKX_ENS_FRONT_MAX_OBJECTIVES;
 * they are read at launch and travel as kernel arguments.  entries[m] = s * n_columns + k as in okx_ensemble_covariance,
 * distinct and in range; sense[m] is OKX_FRONT_MIN, _MAX or _TARGET (then target[m] must be finite; target may be NULL
 * when no objective aims at one).
 * Geometry g is a CANDIDATE when d_mask is NULL or d_mask[g * mask_stride] == 0 - exactly the flag byte
 * okx_ensemble_screen writes, 0 meaning pass - and every selected entry of g counts (complete cases, the rule of the
 * covariance pass).  Its objective o_m is v (MIN), -v (MAX) or |v - target_m| (TARGET, the subtraction rounded once) of the
 * table value v.  a DOMINATES b when o_a[m] <= o_b[m] for every m and o_a[m] < o_b[m] for some m, compared as IEEE values
 * (-0.0 == +0.0).  Candidates with equal objective vectors do not dominate each other: all of them are on the front or none.
 *   d_dominated [n_geometries] int32   the number of candidates of THIS call that dominate g; -1: g is no candidate;
 *                                      0: g is on the front.  With one objective: the competition rank minus one.
 *   d_tally [3] int64                  geometries seen, candidates, front members (the last may exceed capacity)
 *   d_front_index [capacity] int64, d_front_values [capacity][n_objectives] double   (each may be NULL)
 *                                      the front members in ascending row order: d_index[g] when d_index is given,
 *                                      geometry_offset + g otherwise, and the RAW table values of the selected entries,
 *                                      exact bits.  Slots at or beyond capacity, and beyond the count, are never written.
 * Only comparisons and integer counts: no tolerance, no floating-point atomic, bit-identical from run to run and across
 * chunks, devices and ranks, and fronts merge: front(A u B) = front(front(A) u front(B)) - run the pass again over the
 * front_values rows of two calls (steps = 1, n_columns = n_objectives, the same senses and targets, the ids through d_index,
 * a mask for the unused slots).  Launch-only, stream-ordered, no host read-back, no allocation, legal inside a stream
 * capture.  n_geometries = 0 is legal and writes a zero tally.  The pass is O(G^2 M): n_geometries above
 * OKX_ENS_FRONT_MAX_GEOMETRIES is OKX_ERR_INVALID - the cap bounds how long one launch occupies the card; larger ensembles go
 * in chunks and merge.  okx_ensemble_front_check validates the host arguments without a launch (an entry out of range or
 * repeated, a sense outside 0 .. 2, a TARGET objective with a missing or non-finite target, a count outside 1 .. 8,
 * n_geometries above the cap: OKX_ERR_INVALID with okx_last_error text); the launch runs it too.
 */
enum { OKX_FRONT_MIN = 0, OKX_FRONT_MAX = 1, OKX_FRONT_TARGET = 2,
       OKX_ENS_FRONT_MAX_OBJECTIVES = 8, OKX_ENS_FRONT_MAX_GEOMETRIES = 65536 };

int32_t okx_ensemble_front(int64_t n_geometries, int64_t steps, int32_t n_columns,
                           const double* d_values, int64_t ld,
                           const uint8_t* d_status, int64_t status_stride,   /* or NULL                                   */
                           const int32_t* entries, const int32_t* sense,     /* HOST [n_objectives]                       */
                           const double* target, int32_t n_objectives,       /* HOST [n_objectives] or NULL               */
                           const uint8_t* d_mask, int64_t mask_stride,       /* or NULL                                   */
                           const int64_t* d_index, int64_t geometry_offset,  /* d_index [n_geometries] or NULL            */
                           int32_t* d_dominated,                             /* [n_geometries]                            */
                           int64_t* d_tally,                                 /* [3]                                       */
                           int64_t* d_front_index, double* d_front_values,   /* [capacity], [capacity][n_objectives], or NULL */
                           int64_t capacity,
                           void* d_scratch, size_t scratch_bytes, void* stream);
size_t okx_ensemble_front_scratch_bytes(int64_t n_geometries, int32_t n_objectives);
/* host only */
int32_t okx_ensemble_front_check(int64_t n_geometries, int64_t steps, int32_t n_columns,
                                 const int32_t* entries, const int32_t* sense,
                                 const double* target, int32_t n_objectives);

/*
 * Ensemble sampler on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): the head of the ensemble
 * chain - the hardpoint table [n_geometries][n_points][3] that okx_rebind_design reads, drawn in HBM by a COUNTER-BASED
 * generator.  Geometry g's draw is a pure function of (seed, g, latent index, attempt): any chunk, device or rank writes the
 * same bits for the rows [geometry_offset, geometry_offset + n_geometries) it asks for.  The definition is
 * open_kinematics_amd/ensemble_sample.py (NumPy); the pass equals it bit for bit in all four outputs - integer arithmetic and
 * fp64 add, multiply, divide and sqrt, each rounded on its own (no fused multiply-add, no libm call).
 *
 * BITS.  Philox4x32-10 with key = (seed & 0xffffffff, seed >> 32) and the counter words
 *   c0 = g & 0xffffffff      c1 = g >> 32      c2 = latent index z      c3 = attempt | purpose << 8
 * (g the GLOBAL geometry index, attempt 0 .. 15 in bits 0-7, purpose in bits 8-15, bits 16-31 zero).  OKX_SAMPLE_PURPOSE_DRAW:
 * output words w0, w1 give 52 bits k = w0 << 20 | w1 >> 12 and u' = (k + 0.5) * 2^-52, exact and never 0 or 1 (w2, w3 are
 * unused).  OKX_SAMPLE_PURPOSE_STRATA (c0 = c1 = 0, attempt 0): the four output words are the round keys of latent z's
 * stratum permutation.
 * STRATA.  OKX_SAMPLE_IID: u = u'.  OKX_SAMPLE_LHS: u = (pi_z(g) + u') / n_total, one rounded add and one rounded divide,
 * clamped into [2^-53, 1 - 2^-53]; pi_z is a bijection of [0, n_total), n_total <= 2^32: a four-round Feistel network on b
 * bits (the smallest even b >= 2 with 2^b >= n_total), L, R <- R, L ^ (mix(R + key_r) & (2^(b/2) - 1)), walked until the value
 * is below n_total; mix is x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16 on 32 bits.  A redraw
 * keeps pi_z(g) and draws u' again, so every stratum of every latent holds exactly one geometry of the whole ensemble.
 * KINDS (d_kind [n_latents]).  OKX_SAMPLE_UNIFORM: 2 u - 1.  OKX_SAMPLE_NORMAL: the inverse normal CDF of u by Wichura's
 * AS241 (PPND16, within 1e-12 of the true value), Horner sums, the tail's logarithm by exponent split and a polynomial.
 * OKX_SAMPLE_TRUNCATED to [-k, k]: the same of Phi(-k) + u (Phi(k) - Phi(-k)), clamped into [-k, k].  d_bound is
 * [n_latents][3] = k, Phi(-k), Phi(k) - Phi(-k), the two constants computed by the caller (ignored for the other kinds).
 * DELTA.  With d_mixing [n_coords][n_latents]: delta_f = sum over z ascending from 0.0 of mixing[f][z] * latent_z.  Without
 * (NULL; then n_latents == n_coords): delta_f = d_scale[f] * latent_f.  The row is d_nominal [n_points][3] with
 * nominal[c] + delta_f at the flat index c = d_coords[f] = point * 3 + axis (distinct, in range).
 * GUARDS (HOST array of n_guards <= 16 items; they travel as kernel arguments).  OKX_SAMPLE_GUARD_SIGN: sign * row[a] > eps,
 * a a flat coordinate index.  _DISTINCT: points a and b are more than eps apart.  _OFF_LINE: a and b are, and point c is more
 * than eps from the line through them.  Attempt 0, 1, ... enter the counter; the first attempt every guard accepts is kept.
 *   d_hardpoints [n_geometries][n_points][3]
 *   d_latents [n_geometries][n_latents], d_delta [n_geometries][n_coords], d_flags [n_geometries] uint8   (each may be NULL)
 *        flags bit 0: no attempt was valid and the last one stands - the sense of the screen's flag byte, so the table can be
 *        the mask of okx_ensemble_front; bits 4-7: the attempt that was kept.
 * Launch-only, stream-ordered, no host read-back, no allocation, legal inside a stream capture; n_geometries = 0 is legal.
 * okx_ensemble_sample_check validates HOST copies of the tables without a launch (a coordinate out of range or repeated, an
 * unknown kind, a TRUNCATED bound - the k alone, [n_latents] - that is not finite and greater than 0, counts over the caps,
 * a bad guard, n_total over 2^32 or geometry_offset + n_geometries > n_total under LHS: OKX_ERR_INVALID with okx_last_error
 * text); the launch repeats the checks that need no device table, and the kernel never writes outside a row.
 */
enum { OKX_SAMPLE_NORMAL = 0, OKX_SAMPLE_UNIFORM = 1, OKX_SAMPLE_TRUNCATED = 2,
       OKX_SAMPLE_IID = 0, OKX_SAMPLE_LHS = 1,
       OKX_SAMPLE_GUARD_SIGN = 0, OKX_SAMPLE_GUARD_DISTINCT = 1, OKX_SAMPLE_GUARD_OFF_LINE = 2,
       OKX_SAMPLE_PURPOSE_DRAW = 0, OKX_SAMPLE_PURPOSE_STRATA = 1, OKX_SAMPLE_PURPOSE_BOOTSTRAP = 2,
       OKX_ENS_SAMPLE_MAX_COORDS = 288, OKX_ENS_SAMPLE_MAX_LATENTS = 288,
       OKX_ENS_SAMPLE_MAX_GUARDS = 16, OKX_ENS_SAMPLE_MAX_ATTEMPTS = 16 };

typedef struct okx_sample_guard {
  int32_t kind;      /* OKX_SAMPLE_GUARD_*                                                          */
  int32_t a, b, c;   /* SIGN: a = flat coordinate index; DISTINCT: points a, b; OFF_LINE: a, b, c   */
  double eps;
  double sign;       /* SIGN: +1 or -1                                                              */
} okx_sample_guard;

int32_t okx_ensemble_sample(int64_t n_geometries, int64_t geometry_offset, int64_t n_total, uint64_t seed,
                            int32_t n_points, const double* d_nominal,         /* [n_points][3]                           */
                            const int32_t* d_coords, int32_t n_coords,         /* [n_coords]                              */
                            const int32_t* d_kind, const double* d_bound,      /* [n_latents], [n_latents][3]             */
                            int32_t n_latents,
                            const double* d_mixing, const double* d_scale,     /* [n_coords][n_latents] or NULL, [n_coords] */
                            const okx_sample_guard* guards, int32_t n_guards,  /* HOST [n_guards] or NULL                 */
                            int32_t stratify, int32_t max_attempts,
                            double* d_hardpoints,                              /* [n_geometries][n_points][3]             */
                            double* d_latents, double* d_delta, uint8_t* d_flags, /* or NULL                              */
                            void* stream);
/* host only */
int32_t okx_ensemble_sample_check(int64_t n_geometries, int64_t geometry_offset, int64_t n_total, int32_t n_points,
                                  const int32_t* coords, int32_t n_coords,
                                  const int32_t* kind, const double* bound, int32_t n_latents, int32_t has_mixing,
                                  const okx_sample_guard* guards, int32_t n_guards,
                                  int32_t stratify, int32_t max_attempts);

/*
 * Pick-freeze families on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): the structured
 * ensemble a variance decomposition (okx_ensemble_sobol) needs, drawn by the sampler above with ONE counter word changed.
 * d_group [n_latents] int32 puts every latent into a factor group in [0, n_groups), or -1: never swapped;
 * 1 <= n_groups <= OKX_ENS_SOBOL_MAX_GROUPS and every group holds a latent.  A family has M = n_groups + 2 members and
 * geometry g is member b = g % M of family i = g / M (interleaved: a family's rows are contiguous, a chunk of whole families
 * is self-contained): member 0 is A, member 1 is B, member 2 + j is A with the latents of group j taken from B.
 * Latent z of geometry g is the draw of SOURCE ROW src = 2 i + s, always at attempt 0 - the Philox counter
 * (src lo, src hi, z, 0 | OKX_SAMPLE_PURPOSE_DRAW << 8) - with s = 1 when b == 1, or when b >= 2 and d_group[z] == b - 2,
 * else 0.  Under OKX_SAMPLE_LHS the stratum is pi_z(src) over 2 n_families strata: A and B together are one Latin hypercube
 * of the source ensemble.  Kinds, mixing / scale, delta, the row and the guards are those of okx_ensemble_sample; there is
 * one attempt (a redraw of one member would break the coordinates it shares with the others), so d_flags[g] is 1 when a
 * guard fails and 0 otherwise - bits 4-7 are always 0.  Members 0 and 1 of family i are rows 2 i and 2 i + 1 of
 * okx_ensemble_sample with n_total = 2 n_families, bit for bit, and any range of geometries carries the bits of the whole.
 * Launch-only, stream-ordered, no allocation, legal inside a stream capture; n_geometries = 0 is legal.
 * okx_ensemble_sample_families_check validates HOST copies (what okx_ensemble_sample_check does, a group outside
 * [-1, n_groups), a group without a latent, n_groups outside the cap, max_attempts other than 1, under LHS a range beyond
 * the n_families families: OKX_ERR_INVALID with okx_last_error text).
 */
enum { OKX_ENS_SOBOL_MAX_GROUPS = 288 };

int32_t okx_ensemble_sample_families(int64_t n_geometries, int64_t geometry_offset, int64_t n_families, uint64_t seed,
                                     int32_t n_points, const double* d_nominal,
                                     const int32_t* d_coords, int32_t n_coords,
                                     const int32_t* d_kind, const double* d_bound,
                                     int32_t n_latents,
                                     const double* d_mixing, const double* d_scale,
                                     const int32_t* d_group, int32_t n_groups,            /* [n_latents]                 */
                                     const okx_sample_guard* guards, int32_t n_guards,    /* HOST [n_guards] or NULL     */
                                     int32_t stratify,
                                     double* d_hardpoints,
                                     double* d_latents, double* d_delta, uint8_t* d_flags, /* or NULL                    */
                                     void* stream);
/* host only */
int32_t okx_ensemble_sample_families_check(int64_t n_geometries, int64_t geometry_offset, int64_t n_families, int32_t n_points,
                                           const int32_t* coords, int32_t n_coords,
                                           const int32_t* kind, const double* bound, int32_t n_latents, int32_t has_mixing,
                                           const int32_t* group, int32_t n_groups,
                                           const okx_sample_guard* guards, int32_t n_guards,
                                           int32_t stratify, int32_t max_attempts);

/*
 * Sobol' accumulators on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): the variance
 * decomposition of an evaluated pick-freeze ensemble, per (step, column) entry of the table [n_families * M * steps][ld],
 * M = n_groups + 2, laid out as okx_ensemble_sample_families draws it (geometry g = i M + b).  A member COUNTS at an entry by
 * the rule of okx_ensemble_reduce (status & 7 == 1 and a finite value) and, with d_mask [n_families * M] uint8, when bit 0
 * of its byte is clear (the sampler's d_flags).  A family counts at an entry when all M members do; otherwise it is dropped
 * for that entry alone.  With dA, dB, dj = value - d_shift[step][column] of members 0, 1 and 2 + j,
 * d_acc [steps][n_columns][OKX_SOBOL_FIELDS + 3 n_groups], every field a double, sums over the families that count:
 *   OKX_SOBOL_COUNT, OKX_SOBOL_DROPPED        families that count / do not
 *   OKX_SOBOL_SUM_A, OKX_SOBOL_SUM_B          sum dA, sum dB
 *   OKX_SOBOL_SUMSQ_A, OKX_SOBOL_SUMSQ_B      sum dA dA, sum dB dB
 *   OKX_SOBOL_FIELDS + 3 j + 0 / 1 / 2        P_j = sum dB (dj - dA), Q_j = sum (dA - dj)^2, R_j = sum (dB - dj)^2
 * Every difference and product is rounded on its own (no fused multiply-add) and there is no floating-point atomic: partial
 * sums go per slab of families into d_scratch (okx_ensemble_sobol_scratch_bytes), families ascending inside a slab, slabs
 * merged ascending, the slab count from the sizes alone - bit-identical from run to run and from device to device.
 * accumulate = 1 adds into what d_acc holds (all partials need ONE shift); chunkings agree to rounding, exactly when the
 * sums are exact.  The host turns the fields into first-order (Saltelli 2010, Jansen) and total-order (Jansen) indices
 * (ensemble_stats.SobolAccumulator.finalize).  Launch-only, stream-ordered, no allocation, legal inside a stream capture;
 * n_families = 0 leaves zeros (or, accumulating, what was there).  Errors (okx_last_error text): a negative count,
 * ld < n_columns or a null table, n_groups outside [1, OKX_ENS_SOBOL_MAX_GROUPS], too many entries for one call, short
 * scratch.
 */
enum { OKX_SOBOL_COUNT = 0, OKX_SOBOL_DROPPED = 1, OKX_SOBOL_SUM_A = 2, OKX_SOBOL_SUM_B = 3, OKX_SOBOL_SUMSQ_A = 4,
       OKX_SOBOL_SUMSQ_B = 5, OKX_SOBOL_FIELDS = 6 };

int32_t okx_ensemble_sobol(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns,
                           const double* d_values, int64_t ld,              /* [n_families * M * steps][ld]           */
                           const uint8_t* d_status, int64_t status_stride,  /* or NULL                                */
                           const uint8_t* d_mask,                           /* [n_families * M] or NULL               */
                           const double* d_shift,                           /* [steps][n_columns]                     */
                           int32_t accumulate,
                           double* d_acc,                                   /* [steps][n_columns][6 + 3 n_groups]     */
                           void* d_scratch, size_t scratch_bytes, void* stream);
size_t okx_ensemble_sobol_scratch_bytes(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns);

/*
 * Poisson bootstrap weights on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): what a
 * bootstrap of an ensemble statistic resamples with.  Replicate r gives GLOBAL row i (for the Sobol' pass a row is a
 * family) an independent Poisson(1) weight that is a pure function of (seed, i, r), so every chunk, device and rank forms
 * the same replicates and their accumulators merge by addition.  The sampler's generator with its purpose word changed:
 *   u = word r % 4 of Philox4x32-10, key = (seed & 0xffffffff, seed >> 32),
 *       counter = (i & 0xffffffff, i >> 32, r / 4, OKX_SAMPLE_PURPOSE_BOOTSTRAP << 8)
 *   w = the number of k in 0 .. 12 with u >= T[k],   T[k] = floor(2^32 sum over j <= k of e^-1 / j!):
 *       0x5e2d58d8 0xbc5ab1b1 0xeb715e1d 0xfb239797 0xff1025f5 0xffd90f3b 0xfffa8b71
 *       0xffff540c 0xffffed1f 0xfffffe21 0xffffffd4 0xfffffffc 0xffffffff
 * Integers only: the pass equals ensemble_stats.bootstrap_weights (NumPy) byte for byte, and w <= 13.
 *   d_weights [n_rows][n_replicates] uint8, row i = row_offset + its index
 * 1 <= n_replicates <= OKX_ENS_BOOTSTRAP_MAX_REPLICATES (1024).  Launch-only, stream-ordered, no allocation, legal inside
 * a stream capture; n_rows = 0 is legal.  Errors (okx_last_error text): a negative count or offset, n_replicates outside
 * the cap, a null table, too many rows for one call.
 */
enum { OKX_ENS_BOOTSTRAP_MAX_REPLICATES = 1024, OKX_ENS_BOOTSTRAP_MAX_WEIGHT = 13 };

int32_t okx_ensemble_bootstrap_weights(int64_t n_rows, int64_t row_offset, uint64_t seed, int32_t n_replicates,
                                       uint8_t* d_weights,                    /* [n_rows][n_replicates]                */
                                       void* stream);

/*
 * Bootstrap replicates of the Sobol' accumulators on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols
 * up): how far to trust the indices of okx_ensemble_sobol.  Table, counting rule, d_mask and d_shift are exactly those of
 * okx_ensemble_sobol; replicate r holds its fields with every family's term multiplied by the family's weight
 * w = weight of GLOBAL family family_offset + i in replicate r (okx_ensemble_bootstrap_weights with the same seed):
 *   d_acc [n_replicates][steps][n_columns][OKX_SOBOL_FIELDS + 3 n_groups]
 *   COUNT_r = sum w over the families that count, DROPPED_r = sum w over those that do not, SUM_A_r = sum w dA, ...,
 *   P_j,r = sum w (dB (dj - dA)), Q_j,r = sum w (dA - dj)^2, R_j,r = sum w (dB - dj)^2
 * FAMILIES are resampled as independent units.  Under OKX_SAMPLE_LHS they are not quite independent (the strata spread
 * them more evenly than independent draws would), so the intervals the host forms from the replicates
 * (ensemble_stats.SobolBootstrapAccumulator.finalize) are on the conservative side.
 * ROUNDING.  A term is formed as okx_ensemble_sobol forms it (every difference and product rounded on its own), then
 * multiplied by (double)w, rounded, then added, rounded; a family whose weight is 0 in a replicate is skipped there.
 * Families ascend inside a slab, slab partials (d_scratch, okx_ensemble_sobol_bootstrap_scratch_bytes) merge in ascending
 * order after what d_acc holds when accumulate = 1, the slab plan comes from the sizes alone and there is no
 * floating-point atomic: bit-identical from run to run and from device to device; chunkings (with the right family_offset)
 * agree to rounding, exactly when the sums are exact.  d_scratch also takes the weights of the call and one counting byte
 * per (family, entry).  Launch-only, stream-ordered, no allocation, legal inside a stream capture; n_families = 0 leaves
 * zeros (or, accumulating, what was there).  Errors (okx_last_error text): what okx_ensemble_sobol reports, a negative
 * family_offset, n_replicates outside [1, OKX_ENS_BOOTSTRAP_MAX_REPLICATES], too many entries for one call, short scratch.
 */
int32_t okx_ensemble_sobol_bootstrap(int64_t n_families, int64_t family_offset, int32_t n_groups, int64_t steps, int32_t n_columns,
                                     const double* d_values, int64_t ld,              /* [n_families * M * steps][ld]  */
                                     const uint8_t* d_status, int64_t status_stride,  /* or NULL                       */
                                     const uint8_t* d_mask,                           /* [n_families * M] or NULL      */
                                     const double* d_shift,                           /* [steps][n_columns]            */
                                     uint64_t seed, int32_t n_replicates, int32_t accumulate,
                                     double* d_acc,            /* [n_replicates][steps][n_columns][6 + 3 n_groups]     */
                                     void* d_scratch, size_t scratch_bytes, void* stream);
size_t okx_ensemble_sobol_bootstrap_scratch_bytes(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns,
                                                  int32_t n_replicates);

/*
 * Main effects from given data on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): how every
 * (step, column) entry of an evaluated ensemble depends on ONE factor beyond a straight line - its conditional moments over
 * equal-probability bins of the factor (Plischke 2010), from the ordinary ensemble that is already in HBM, without a further
 * solve.  Two passes: the factors are binned once (they do not change from step to step), the table is streamed per call.
 *
 * okx_ensemble_bin.  d_factors [n_geometries][ldf] doubles (n_factors <= ldf), d_edges [n_factors][n_bins - 1] the ascending
 * interior edges of every factor's bins (the caller validates them: finite and non-decreasing), 1 <= n_bins <=
 * OKX_ENS_EFFECTS_MAX_BINS, 1 <= n_factors <= OKX_ENS_EFFECTS_MAX_FACTORS.  Outputs:
 *   d_bins    [n_geometries][n_factors] uint8   the bin of the geometry for the factor: the NUMBER OF EDGES <= x - comparisons
 *             only, a value on an edge goes to the upper bin, -inf / +inf land in the end bins; OKX_ENS_EFFECTS_NO_BIN for a NaN
 *             (the geometry is left out for that factor alone)
 *   d_order   [n_factors][n_geometries] int32   per factor its binned geometries, bin by bin, ASCENDING geometry index inside a
 *             bin; the slots behind the last binned geometry hold -1
 *   d_offsets [n_factors][n_bins + 1] int64     where every bin starts in that list; the last entry is the binned count
 * Positions come from ballots and prefix counts, no atomic decides a slot: the same bits every run.  Integers and comparisons
 * only: the pass equals ensemble_stats.bin_factors_host byte for byte.
 *
 * okx_ensemble_effects.  Table, status bytes and counting rule are those of okx_ensemble_reduce (status & 7 == 1 and a finite
 * value); with d_mask [n_geometries] uint8 a geometry counts only when bit 0 of its byte is clear (the sampler's d_flags).
 * d_order / d_offsets are what okx_ensemble_bin made of the SAME geometries.  With d = value - d_shift[step][column],
 *   d_acc [n_factors][n_bins][OKX_EFFECTS_FIELDS][steps * n_columns], every field a double, the entry fastest:
 *   OKX_EFFECTS_COUNT, OKX_EFFECTS_SUM, OKX_EFFECTS_SUMSQ   the geometries of the bin that count at the entry, sum d, sum d d
 * ROUNDING.  d is rounded, then d d, then each is added (no fused multiply-add).  Every cell is ONE chain of additions over the
 * bin's geometries in ascending order, begun at 0 (accumulate = 0; a cell whose bin is empty gets zeros) or at what d_acc
 * holds (accumulate = 1; all partials need ONE shift and the same edges): no slabs, no scratch, no floating-point atomic -
 * bit-identical from run to run and from device to device, equal to ensemble_stats.effects_host on integer tables; chunks
 * accumulated in ascending order carry the bits of the whole, accumulators merged by addition differ from it by the addition
 * order only.  The table is read once per factor.  The host turns the fields into conditional means, within-bin spreads and
 * the first-order indices (ensemble_stats.EffectsAccumulator.finalize).
 * Both are launch-only, stream-ordered, without allocation and legal inside a stream capture; n_geometries = 0 is legal
 * (offsets of zeros; zeros or, accumulating, what was there).  Errors (okx_last_error text): a negative count, n_factors or
 * n_bins outside their caps, ld < n_columns / ldf < n_factors or a null table, more than 2^31 - 1 geometries or too many
 * entries for one call.
 */
enum { OKX_ENS_EFFECTS_MAX_BINS = 64, OKX_ENS_EFFECTS_MAX_FACTORS = 288, OKX_ENS_EFFECTS_NO_BIN = 255 };
enum { OKX_EFFECTS_COUNT = 0, OKX_EFFECTS_SUM = 1, OKX_EFFECTS_SUMSQ = 2, OKX_EFFECTS_FIELDS = 3 };

int32_t okx_ensemble_bin(int64_t n_geometries, int32_t n_factors,
                         const double* d_factors, int64_t ldf,              /* [n_geometries][ldf]                      */
                         const double* d_edges, int32_t n_bins,             /* [n_factors][n_bins - 1]                  */
                         uint8_t* d_bins,                                   /* [n_geometries][n_factors]                */
                         int32_t* d_order,                                  /* [n_factors][n_geometries]                */
                         int64_t* d_offsets,                                /* [n_factors][n_bins + 1]                  */
                         void* stream);

int32_t okx_ensemble_effects(int64_t n_geometries, int64_t steps, int32_t n_columns,
                             const double* d_values, int64_t ld,              /* [n_geometries * steps][ld]           */
                             const uint8_t* d_status, int64_t status_stride,  /* or NULL                              */
                             const uint8_t* d_mask,                           /* [n_geometries] or NULL               */
                             int32_t n_factors, int32_t n_bins,
                             const int32_t* d_order, const int64_t* d_offsets, /* of okx_ensemble_bin                 */
                             const double* d_shift,                           /* [steps][n_columns]                   */
                             int32_t accumulate,
                             double* d_acc,                       /* [n_factors][n_bins][3][steps * n_columns]        */
                             void* stream);

/*
 * Tolerance what-ifs by likelihood reweighting on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up):
 * what the scatter and the yield of an evaluated ensemble BECOME when the law of some latents changes from p to q - a tolerance
 * tightened, a nominal re-centred - from the ensemble that is already in HBM, without a further draw or solve.  A scenario is a
 * per-geometry likelihood ratio w_g = q(z_g) / p(z_g) of the latents the sampler kept (okx_ensemble_sample's d_latents); every
 * what-if statistic is a weighted sum over the evaluated table.
 *
 * okx_ensemble_tilt_weights.  d_latents [n_geometries][ldz] doubles (n_latents <= ldz), d_tilt [n_scenarios][n_latents]
 * [OKX_TILT_PARAMS] = (a, b, c, lo, hi) per (scenario, latent) - ensemble_sample.tolerance_scenarios builds it -,
 * 1 <= n_scenarios <= OKX_ENS_TILT_MAX_SCENARIOS, 1 <= n_latents <= OKX_ENS_SAMPLE_MAX_LATENTS.  Per (geometry, scenario), over
 * the latents z in ascending order:
 *   inside = lo <= z <= hi (comparisons: a NaN latent is outside), term = (c z + b) z + a, logw = 0.0 + term_0 + term_1 + ...
 *   d_weights [n_geometries][ldw] double (n_scenarios <= ldw):  w = every latent inside ? exp_unit(logw) : 0.0
 * exp_unit(x): k = rint(x * 1.4426950408889634), r = (x - k * LN2_HI) - k * LN2_LO with LN2_HI = 0x3fe62e42fee00000 and
 * LN2_LO = 1.9082149292705877e-10, P = the Horner sum of r^n / n!, n = 0 .. 13, the result ldexp(P, k); x < -708 and NaN give
 * 0.0, x > 708 is taken as 708.  Every operation is rounded on its own (contraction is off for the unit): the pass equals
 * ensemble_sample.tilt_weights_host (NumPy) bit for bit.  The launch cannot read d_tilt on the host:
 * okx_ensemble_tilt_check validates a HOST copy of it (a NaN, lo > hi, a non-finite a, b or c, the caps).
 *
 * okx_ensemble_reweigh.  Table, status bytes and counting rule are those of okx_ensemble_reduce (status & 7 == 1 and a finite
 * value); with d_mask [n_geometries] uint8 a geometry counts only when bit 0 of its byte is clear (the sampler's d_flags).
 * d_weights [n_geometries][ldw] the weights of n_scenarios scenarios (the pass above, or any doubles); d_limits
 * [steps][n_columns][2] = (lo, hi) or NULL (nothing is outside); d_verdict [n_geometries] uint8, okx_ensemble_screen's d_flags, or
 * NULL (every geometry passes).  With d = value - d_shift[step][column] and ww = w w:
 *   d_acc [n_scenarios][OKX_REWEIGH_FIELDS][steps * n_columns], every field a double, the entry fastest, over the states that count:
 *   OKX_REWEIGH_COUNT those with w > 0;  OKX_REWEIGH_W sum w;  OKX_REWEIGH_WW sum ww;  OKX_REWEIGH_WD sum w d;
 *   OKX_REWEIGH_WDD sum (w d) d;  OKX_REWEIGH_WWD sum ww d;  OKX_REWEIGH_WWDD sum (ww d) d;  OKX_REWEIGH_OUT_LO sum w [value < lo];
 *   OKX_REWEIGH_OUT_HI sum w [value > hi];  OKX_REWEIGH_WW_OUT sum ww [value < lo or value > hi]
 *   d_joint [n_scenarios][OKX_REWEIGH_JOINT_FIELDS] over the geometries whose mask bit is clear:
 *   OKX_REWEIGH_JOINT_SEEN sum w;  _SEEN_WW sum ww;  _PASS sum w [verdict == 0];  _PASS_WW;  _OUTSIDE sum w [verdict &
 *   OKX_SCREEN_OUTSIDE];  _UNRESOLVED sum w [verdict & OKX_SCREEN_UNRESOLVED];  _GEOMETRIES their number (the same in every scenario)
 * ROUNDING.  d, ww and every product are rounded on their own, then added (no fused multiply-add); a geometry whose weight is
 * 0 in a scenario is skipped there.  Geometries ascend inside a slab, slab partials (d_scratch, okx_ensemble_reweigh_scratch_bytes)
 * merge in ascending order after what d_acc / d_joint hold when accumulate = 1 (all partials need ONE shift and the same
 * limits), the slab plan comes from the sizes alone and there is no floating-point atomic: bit-identical from run to run and
 * from device to device; chunkings agree to rounding, exactly when the sums are exact.  The host turns the fields into
 * self-normalised means, spreads, effective sample sizes, standard errors and yields (ensemble_stats.ReweighAccumulator.finalize).
 * Both are launch-only, stream-ordered, without allocation and legal inside a stream capture; n_geometries = 0 is legal
 * (no weights; zeros or, accumulating, what was there).  Errors (okx_last_error text): a negative count, n_scenarios or
 * n_latents outside their caps, ld < n_columns / ldz < n_latents / ldw < n_scenarios or a null table, too many entries for one
 * call, short or misaligned scratch.
 */
enum { OKX_ENS_TILT_MAX_SCENARIOS = 256, OKX_TILT_PARAMS = 5 };
enum { OKX_REWEIGH_COUNT = 0, OKX_REWEIGH_W = 1, OKX_REWEIGH_WW = 2, OKX_REWEIGH_WD = 3, OKX_REWEIGH_WDD = 4, OKX_REWEIGH_WWD = 5,
       OKX_REWEIGH_WWDD = 6, OKX_REWEIGH_OUT_LO = 7, OKX_REWEIGH_OUT_HI = 8, OKX_REWEIGH_WW_OUT = 9, OKX_REWEIGH_FIELDS = 10 };
enum { OKX_REWEIGH_JOINT_SEEN = 0, OKX_REWEIGH_JOINT_SEEN_WW = 1, OKX_REWEIGH_JOINT_PASS = 2, OKX_REWEIGH_JOINT_PASS_WW = 3,
       OKX_REWEIGH_JOINT_OUTSIDE = 4, OKX_REWEIGH_JOINT_UNRESOLVED = 5, OKX_REWEIGH_JOINT_GEOMETRIES = 6, OKX_REWEIGH_JOINT_FIELDS = 7 };

int32_t okx_ensemble_tilt_weights(int64_t n_geometries,
                                  const double* d_latents, int64_t ldz, int32_t n_latents,  /* [n_geometries][ldz]            */
                                  const double* d_tilt, int32_t n_scenarios,                /* [n_scenarios][n_latents][5]    */
                                  double* d_weights, int64_t ldw,                           /* [n_geometries][ldw]            */
                                  void* stream);
int32_t okx_ensemble_tilt_check(const double* tilt, int32_t n_scenarios, int32_t n_latents);

int32_t okx_ensemble_reweigh(int64_t n_geometries, int64_t steps, int32_t n_columns,
                             const double* d_values, int64_t ld,              /* [n_geometries * steps][ld]           */
                             const uint8_t* d_status, int64_t status_stride,  /* or NULL                              */
                             const uint8_t* d_mask,                           /* [n_geometries] or NULL               */
                             const double* d_shift,                           /* [steps][n_columns]                   */
                             const double* d_weights, int64_t ldw, int32_t n_scenarios, /* [n_geometries][ldw]        */
                             const double* d_limits,                          /* [steps][n_columns][2] or NULL        */
                             const uint8_t* d_verdict,                        /* [n_geometries] or NULL               */
                             int32_t accumulate,
                             double* d_acc,                       /* [n_scenarios][10][steps * n_columns]             */
                             double* d_joint,                     /* [n_scenarios][7]                                 */
                             void* d_scratch, size_t scratch_bytes, void* stream);
size_t okx_ensemble_reweigh_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_scenarios);

/*
 * Polynomial response surface on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): a regression of
 * selected entries of the evaluated table on products of orthonormal polynomials of per-geometry factors (a polynomial chaos
 * expansion of total degree <= 3 with pairwise products) - which PAIRS of factors act together, a model of the table that
 * predicts an entry at a perturbed geometry without a solve, and first-order / pairwise / total variance shares from ONE fit on
 * the ORDINARY ensemble.  The device forms the normal equations; the host solves them (ensemble_stats.SurfaceAccumulator.finalize).
 *
 * okx_ensemble_basis.  d_factors [n_geometries][ld] doubles (n_factors <= ld, 1 <= n_factors <= OKX_ENS_SAMPLE_MAX_LATENTS); d_law
 * [n_factors][3] doubles = (kind, centre, scale), kind OKX_SURFACE_MONOMIAL / _HERMITE / _LEGENDRE; d_terms [n_terms][4] int32 =
 * (a, da, b, db): the term is psi_da(u_a) psi_db(u_b), a factor index -1 (with degree 0) where there is no factor; term 0 is the
 * constant (-1, 0, -1, 0); 1 <= n_terms <= OKX_ENS_SURFACE_MAX_TERMS, degrees 1 .. OKX_ENS_SURFACE_MAX_DEGREE.  Per (geometry, term):
 *   u = (x - centre) * scale, psi_0 = 1, and for degrees 1, 2, 3
 *   monomial  u, u u, (u u) u
 *   Hermite   u, (u u - 1) * 0.7071067811865476, ((u u - 3) * u) * 0.408248290463863
 *   Legendre  u * 1.7320508075688772, (3 (u u) - 1) * 1.118033988749895, ((5 (u u) - 3) * u) * 1.3228756555322954
 *   d_phi   [n_geometries][ld_phi] double (n_terms <= ld_phi): the product of the term's two psi
 *   d_valid [n_geometries] uint8: 0 where ANY of the row's n_factors factors is not finite - that row of d_phi is then 0
 * Every operation is rounded on its own (contraction is off for the unit): the pass equals ensemble_stats.basis_host (NumPy) bit
 * for bit.  The launch cannot read d_law / d_terms on the host: okx_ensemble_basis_check validates HOST copies (counts outside
 * their caps, a kind that is none of the three, a centre or scale that is not finite, a missing constant term, a factor index or
 * degree out of range); on the device a factor index out of range reads as "no factor".
 *
 * okx_ensemble_surface.  Table, status bytes, entry list and shift are those of okx_ensemble_covariance, with a limit of its own:
 * 1 <= n_entries <= OKX_ENS_SURFACE_MAX_ENTRIES.  COMPLETE CASES: a geometry is USED when every selected entry of it counts
 * (status & 7 == 1 and a finite value), bit 0 of its d_mask byte is clear (d_mask [n_geometries] uint8 or NULL: the sampler's
 * d_flags) and its d_valid byte is set.  With phi = d_phi's row (the basis pass, or any doubles), d = value - d_shift[entry] over
 * the used geometries, T = n_terms, N = n_entries:
 *   d_gram   [T][T] double  sum phi_t phi_t', the full square; gram[t][t'] and gram[t'][t] are the same bits
 *   d_cross  [T][N] double  sum phi_t d_n
 *   d_sumsq  [N]    double  sum d_n d_n (the product rounded, then added)
 *   d_counts [2]    int64   geometries used, dropped
 *   d_used   [n_geometries] uint8 or NULL: 1 where geometry g of THIS call is used
 * d_valid says that the FACTORS of a row are finite, not that its basis values are: a finite factor whose u u overflows, or a table
 * of the caller's own with a NaN or inf in a used row, is summed as it lies and leaves inf / NaN in d_gram and d_cross - the row is not
 * dropped.  accumulate = 0 overwrites gram, cross, sumsq and counts; accumulate = 1 adds this call after what they hold - additions only,
 * so it needs the same shift, entries and basis as the calls before.  Launch-only, stream-ordered, no host read-back, no
 * allocation, legal inside a stream capture (one chain of three launches); n_geometries = 0 is legal.  No floating-point
 * atomics (no atomics on device memory at all): the geometries are cut into slabs by a plan that is a function of
 * (n_geometries, n_terms, n_entries) alone and never looks at the device, a slab is summed in ascending geometry order, four at a
 * time in v_mfma_f64_16x16x4_f64, and the slabs are added in ascending order per output element - two runs, or two devices, give
 * the same bits.  DIFFERENT CHUNKINGS of the same geometries agree to rounding only: |result - exact| <= (G + 2) u sum |term| each
 * (exactly where every product and sum is representable).  d_scratch: okx_ensemble_surface_scratch_bytes.  The launch cannot read
 * d_entries on the host: okx_ensemble_surface_check validates a HOST copy (okx_ensemble_covariance_check's rules and words under
 * this pass's name and limits) before it is uploaded; on the device an index out of range is never dereferenced - its entry never
 * counts, every geometry is dropped.
 */
enum { OKX_ENS_SURFACE_MAX_TERMS = 1024, OKX_ENS_SURFACE_MAX_ENTRIES = 2048, OKX_ENS_SURFACE_MAX_DEGREE = 3 };
enum { OKX_SURFACE_MONOMIAL = 0, OKX_SURFACE_HERMITE = 1, OKX_SURFACE_LEGENDRE = 2 };

int32_t okx_ensemble_basis(int64_t n_geometries,
                           const double* d_factors, int64_t ld, int32_t n_factors,  /* [n_geometries][ld]                    */
                           const double* d_law,                                     /* [n_factors][3]                        */
                           const int32_t* d_terms, int32_t n_terms,                 /* [n_terms][4]                          */
                           double* d_phi, int64_t ld_phi,                           /* [n_geometries][ld_phi]                */
                           uint8_t* d_valid,                                        /* [n_geometries]                        */
                           void* stream);
int32_t okx_ensemble_basis_check(const double* law, int32_t n_factors, const int32_t* terms, int32_t n_terms);

int32_t okx_ensemble_surface(int64_t n_geometries, int64_t steps, int32_t n_columns,
                             const double* d_values, int64_t ld,              /* [n_geometries * steps][ld]           */
                             const uint8_t* d_status, int64_t status_stride,  /* or NULL                              */
                             const uint8_t* d_mask,                           /* [n_geometries] or NULL               */
                             const double* d_phi, int64_t ld_phi,             /* [n_geometries][ld_phi]               */
                             const uint8_t* d_valid,                          /* [n_geometries]                       */
                             int32_t n_terms,
                             const int32_t* d_entries, int32_t n_entries,     /* or NULL: all, n_entries = steps * n_columns */
                             const double* d_shift,
                             int32_t accumulate,
                             double* d_gram, double* d_cross, double* d_sumsq, int64_t* d_counts,
                             uint8_t* d_used,                                 /* or NULL                              */
                             void* d_scratch, size_t scratch_bytes, void* stream);
/* host only */
size_t okx_ensemble_surface_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_terms, int32_t n_entries);
int32_t okx_ensemble_surface_check(const int32_t* entries /* or NULL */, int32_t n_entries, int64_t n_table_entries, int32_t n_terms);

/*
 * Evaluation of a response surface on device (ADDED UNDER ABI 6 - nothing existing changed; look the symbols up): the fitted
 * model as a column table that every ensemble pass reads, without the basis table [G][T] ever lying in memory.
 *
 * okx_ensemble_predict.  d_factors, ld, n_factors, d_law, d_terms and n_terms exactly as okx_ensemble_basis takes them, under the
 * same limits; d_coefficients [n_terms][ld_c] doubles with 1 <= n_entries <= OKX_ENS_SURFACE_MAX_ENTRIES columns (n_entries <=
 * ld_c); d_shift [n_entries] doubles or NULL (zeros); d_mask [n_geometries] uint8 or NULL, bit 0 set drops the row (the sampler's
 * d_flags).  With psi_t the basis value of term t (the bits of okx_ensemble_basis), N = n_entries:
 *   mode OKX_PREDICT_VALUE     d_out[g][n] = shift[n] + sum_t psi_t c[t][n]
 *   mode OKX_PREDICT_RESIDUAL  d_out[g][n] = value[g][entry n] - (shift[n] + sum_t psi_t c[t][n])
 *   d_out   [n_geometries][ld_out] double (N <= ld_out); columns at and beyond N are not touched
 *   d_valid [n_geometries] uint8: 0 where ANY of the row's n_factors factors is not finite or bit 0 of its mask byte is set -
 *           that row of d_out is then NaN in every column
 * RESIDUAL mode reads the table the way every ensemble pass takes it (steps, n_columns, d_values, ld_values, d_status,
 * status_stride; d_entries [N] int32 = s * n_columns + k, or NULL: all steps * n_columns = N entries in natural order); an entry
 * that does not count (status & 7 != 1 or a value that is not finite) is NaN.  VALUE mode ignores those seven arguments.
 *
 * THE BITS.  ROW-PURE: the row of a geometry is a function of its factor row, the basis, the coefficients and the shift alone.
 * The sum over the terms starts at 0 and takes the terms in ascending panels of 32 (the terms beyond T are zeros), four at a time in
 * v_mfma_f64_16x16x4_f64 - an order that depends on n_terms only: not on n_geometries, not on where the row lies in the call,
 * not on ld, ld_c, ld_out or n_entries, not on what else runs.  Then the shift is added in ONE rounded addition, then (RESIDUAL)
 * the difference is taken in ONE rounded subtraction.  So every chunking, every device and every rank gives a geometry the same
 * bits, and a chunk that is drawn and predicted again is the same chunk.  Against exact arithmetic:
 * |out - exact| <= (T + 4) u (|shift| + sum_t |psi_t c_t|) + 2 u |value|, u = 2^-53, with psi_t the basis values as rounded.
 * One launch on the given stream, no scratch, no atomics, no allocation, no host read-back: legal inside a stream capture;
 * n_geometries = 0 is legal.  The launch cannot read d_entries on the host: okx_ensemble_predict_check validates a HOST copy
 * (the counts; with n_table_entries > 0 the entry list by okx_ensemble_surface_check's rules and words under this pass's name);
 * the law and the terms are validated by okx_ensemble_basis_check.  On the device an entry index out of range is never
 * dereferenced (its column is NaN) and a factor index out of range reads as "no factor".
 */
enum { OKX_PREDICT_VALUE = 0, OKX_PREDICT_RESIDUAL = 1 };

int32_t okx_ensemble_predict(int64_t n_geometries, int32_t mode,
                             const double* d_factors, int64_t ld, int32_t n_factors,  /* [n_geometries][ld]                    */
                             const double* d_law,                                     /* [n_factors][3]                        */
                             const int32_t* d_terms, int32_t n_terms,                 /* [n_terms][4]                          */
                             const double* d_coefficients, int64_t ld_c, int32_t n_entries, /* [n_terms][ld_c]                 */
                             const double* d_shift,                                   /* [n_entries] or NULL                   */
                             const uint8_t* d_mask,                                   /* [n_geometries] or NULL                */
                             int64_t steps, int32_t n_columns,                        /* RESIDUAL: the table ...               */
                             const double* d_values, int64_t ld_values,               /* [n_geometries * steps][ld_values]     */
                             const uint8_t* d_status, int64_t status_stride,          /* or NULL                               */
                             const int32_t* d_entries,                                /* [n_entries] or NULL                   */
                             double* d_out, int64_t ld_out,                           /* [n_geometries][ld_out]                */
                             uint8_t* d_valid,                                        /* [n_geometries]                        */
                             void* stream);
/* host only */
int32_t okx_ensemble_predict_check(const int32_t* entries /* or NULL */, int32_t n_entries, int64_t n_table_entries, int32_t n_terms,
                                   int32_t n_factors);

#ifdef __cplusplus
}
#endif
#endif /* OKX_H */
