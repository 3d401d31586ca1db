// Which ReactiveQPController kernel serves a batch: the plan of the reduced QP and the shape predicates the
// shape-specialised kernels are built on (make_qp_plan, the box and mixed families, the LDS slot layout), the inputs of
// the choice (QpPolicy, QpKernels), the ONE function that makes it (qp_select) and the launchers' signatures.  No
// kernels here: the library's host code (clik_api.hip) includes it as well as the kernels (clik_qp_static.hpp).
#pragma once
#include <cstdlib>
#include "clik_device.hpp"

namespace clik {

constexpr size_t kLdsBytesPerCu = 160u * 1024u;     // LDS of one CU (gfx950)

// ---- compile-time plan of the reduced QP ---------------------------------------------
constexpr int QPS_MAX_ROWS = 16;       // active-set rows a static QP kernel carries in registers

struct QpPlanS {
    int  nr;                               // rows handed to the active-set solver
    int  row_task[CLIK_MAX_QPROWS];
    int  row_local[CLIK_MAX_QPROWS];
    int  ns;                               // slack variables (= soft rows, in row order)
    int  slack_base[SHAPE_MAX_TASKS];      // first slack of a soft task
    bool folded[SHAPE_MAX_TASKS];          // soft equality: eliminated into P, g
    // active-set row of output i of a task that is not folded, and whether it shares that row with an
    // earlier constraint: two hard joint-space rows on the same state (joint limits  lb <= dq_i <= ub  from a
    // SetConstraint on q and the speed limit  -v <= dq_i <= v  of a VelocitySetConstraint on q - the pair
    // every UR5 notebook stacks, e.g. ur5_dual_quaternion_vs_transformation_matrix.ipynb cell 14) are ONE
    // row  max(lb) <= dq_i <= min(ub): same feasible set, same minimiser, half the active-set size.
    int  row_of[SHAPE_MAX_TASKS][CLIK_MAX_M];
    bool merged[SHAPE_MAX_TASKS][CLIK_MAX_M];
};

constexpr QpPlanS make_qp_plan(const ShapeDesc& sd)
{
    QpPlanS p{};
    for (int ti = 0; ti < sd.n_tasks; ++ti) {
        const int cls = sd.cls[ti];
        const bool soft = sd.soft[ti] != 0;
        p.slack_base[ti] = p.ns;
        if (soft) p.ns += sd.m[ti];
        p.folded[ti] = soft && (cls == CLIK_CLS_EQ || cls == CLIK_CLS_VELEQ);
        if (!p.folded[ti]) {
            const bool box = !soft && shape_unit(sd, ti) && (cls == CLIK_CLS_SET || cls == CLIK_CLS_VELSET);
            for (int i = 0; i < sd.m[ti]; ++i) {
                int same = -1;
                if (box)
                    for (int r = 0; r < p.nr && r < CLIK_MAX_QPROWS && same < 0; ++r) {
                        const int t2 = p.row_task[r];
                        const bool box2 = sd.soft[t2] == 0 && shape_unit(sd, t2) &&
                                          (sd.cls[t2] == CLIK_CLS_SET || sd.cls[t2] == CLIK_CLS_VELSET);
                        if (box2 && sd.ucol[t2][p.row_local[r]] == sd.ucol[ti][i]) same = r;
                    }
                if (same >= 0) {
                    p.row_of[ti][i] = same;
                    p.merged[ti][i] = true;
                    continue;
                }
                p.row_of[ti][i] = p.nr;
                if (p.nr < CLIK_MAX_QPROWS) {
                    p.row_task[p.nr] = ti;
                    p.row_local[p.nr] = i;
                }
                ++p.nr;
            }
        }
    }
    return p;
}

// Box family: after the soft equalities are folded into P and g, every remaining row is a HARD bound on one state
// variable (joint-limit SetConstraint / speed-limit VelocitySetConstraint on q, merged per state):
//     min 1/2 v'P v - g'v   s.t.  lb_c <= v_c <= ub_c  on the bounded states c
// (BASELINE config 4 and the QP stacks of the UR5 notebooks).  Such a QP is solved by a primal active-set
// iteration on the states (qp_box_pas) instead of the dual active-set iteration over rows.
constexpr bool qp_box_family(const ShapeDesc& sd)
{
    const QpPlanS p = make_qp_plan(sd);
    if (p.nr <= 0 || p.nr > CLIK_MAX_DOF) return false;
    for (int r = 0; r < p.nr; ++r) {
        const int ti = p.row_task[r];
        if (sd.soft[ti] != 0 || !shape_unit(sd, ti)) return false;
        if (sd.cls[ti] != CLIK_CLS_SET && sd.cls[ti] != CLIK_CLS_VELSET) return false;
    }
    return true;
}
// Solvers measured for this family on config 4 (16384 instances, cold / hot start per tick, same box):
//   dual active-set iteration over rows (gi_solve, what every other QP shape runs)      38.7 / 10.4 us
//   projected Newton (round 2, tools/experiments/qp_retired.patch)                      38.5 / 25.8 us
//   block principal pivoting (first attempt, history)                                   93   /  7.4 us
//   primal active set from the vertex the linear term points to, qp_box_pas (default)   see DESIGN.md section 5
// The tick is the slowest instance of the batch (every wave has a SIMD to itself), i.e. its pass count times the
// instructions of a pass: the dual iteration needs 11-13 passes of ~1000 instructions on the worst instance, the
// projected Newton 10 of ~1500, the primal active set up to 19 of ~350 (mean 3.3): only 0-3 of the 7 states are
// free at the optimum, so a method that starts from a vertex and frees one state per pass is there quickly, and
// a pass is one masked 7 x 7 factorisation with everything in registers.  -DCLIK_QP_BOX_OFF: this family runs the
// dual iteration like the others (regression switch).
#if defined(CLIK_QP_BOX_OFF)
#define CLIK_QP_BOX_OK(SD) false
#else
#define CLIK_QP_BOX_OK(SD) qp_box_family(SD)
#endif

// Mixed family (round 3): the rows left after folding are hard bounds on single states (the box), a few HARD
// GENERAL rows (a SetConstraint on a task-space expression - the wall sets of ur5_moe2016_example2.ipynb cell 6 -
// reactive_qp.py:221-225; hard equalities), and SOFT inequality rows.  A soft inequality row  lb <= a v - s <= ub
// with cost 1/2 h s^2  is exactly a bounded variable  w = a v - s in [lb, ub]  with cost  1/2 h (a v - w)^2: it is
// LIFTED into the box (z = [v; w]).  The hard general rows enter a primal active set next to the held states
// (qp_mixed_pas).  Row kinds, in plan order:
constexpr int QPK_BOX = 0, QPK_HARD = 1, QPK_LIFT = 2;
#ifndef CLIK_QP_MIXED_MAX_Z
#define CLIK_QP_MIXED_MAX_Z 8          // states + lifted rows carried in registers
#endif
#ifndef CLIK_QP_MIXED_MAX_H
#define CLIK_QP_MIXED_MAX_H 3          // hard general rows
#endif
constexpr int qp_row_kind(const ShapeDesc& sd, const QpPlanS& p, int r)
{
    const int ti = p.row_task[r];
    if (sd.soft[ti] != 0) return QPK_LIFT;
    if (shape_unit(sd, ti) && (sd.cls[ti] == CLIK_CLS_SET || sd.cls[ti] == CLIK_CLS_VELSET)) return QPK_BOX;
    return QPK_HARD;
}
constexpr int qp_kind_count(const ShapeDesc& sd, int kind)
{
    const QpPlanS p = make_qp_plan(sd);
    int n = 0;
    for (int r = 0; r < p.nr && r < CLIK_MAX_QPROWS; ++r) n += qp_row_kind(sd, p, r) == kind;
    return n;
}
// index of row r among the rows of its kind
constexpr int qp_kind_index(const ShapeDesc& sd, int r)
{
    const QpPlanS p = make_qp_plan(sd);
    const int kind = qp_row_kind(sd, p, r);
    int n = 0;
    for (int q = 0; q < r; ++q) n += qp_row_kind(sd, p, q) == kind;
    return n;
}
constexpr bool qp_mixed_family(const ShapeDesc& sd)
{
    const QpPlanS p = make_qp_plan(sd);
    if (p.nr <= 0 || p.nr > CLIK_MAX_QPROWS || qp_box_family(sd)) return false;
    const int nl = qp_kind_count(sd, QPK_LIFT), nh = qp_kind_count(sd, QPK_HARD);
    if (nl + nh == 0) return false;
    // (skills with generated attribute code keep the dual iteration: its row bounds come through another path)
    // (registers: the packed matrix and its factor dominate - without hard rows one more variable fits;
    // measured on the 6-DoF + 3 soft walls skill: 256 VGPRs + 155 AGPRs, no scratch)
    return sd.n + nl <= CLIK_QP_MIXED_MAX_Z + (nh == 0 ? 1 : 0) && nh <= CLIK_QP_MIXED_MAX_H;
}
#if defined(CLIK_QP_MIXED_OFF) || defined(CLIK_QP_BOX_OFF)
#define CLIK_QP_MIXED_OK(SD) false
#else
#define CLIK_QP_MIXED_OK(SD) qp_mixed_family(SD)
#endif

// 64-double LDS slots a shape-specialised QP kernel keeps behind the skill image (QpLayout reads its offsets from here,
// the library's eligibility test its slot count): the primal families (bound-constrained, mixed) keep no dual Hessian
// Q, no P^-1 a_r' and no c0 there, so a two-arm skill with 14 merged box rows fits where the dual form's would not
struct QpSlotLayout {
    int o_z, o_y, o_q, o_lb, o_ub, o_c0, o_ys, o_sl;
    int slots;
};
constexpr QpSlotLayout qp_slot_layout(const ShapeDesc& sd)
{
    const QpPlanS p = make_qp_plan(sd);
    const bool primal = CLIK_QP_BOX_OK(sd) || CLIK_QP_MIXED_OK(sd);
    const int n = sd.n, ny = sd.n_y > 0 ? sd.n_y : 0, nra = p.nr > 0 ? p.nr : 1, nsa = p.ns > 0 ? p.ns : 1;
    const int nt = nra * (nra + 1) / 2;
    QpSlotLayout l{};
    l.o_z = 0;
    l.o_y = l.o_z + n;
    l.o_q = l.o_y + ny;
    l.o_lb = l.o_q + (primal ? 0 : nt);
    l.o_ub = l.o_lb + nra;
    l.o_c0 = l.o_ub + nra;
    l.o_ys = l.o_c0 + (primal ? 0 : nra);        // P^-1 a_r'  (NR x N)
    l.o_sl = l.o_ys + (primal ? 0 : nra * n);    // folded right-hand sides, then the slack output rows
    l.slots = l.o_sl + nsa;
    return l;
}

// the bound-constrained skills whose sin / cos evaluations four lanes per instance can share ("front4") ...
constexpr bool qp_front4_ok(const ShapeDesc& sd) { return CLIK_QP_BOX_OK(sd) && sd.uses_fk != 0 && sd.n >= 3 && sd.n <= 8; }
// ... and those of them with a resident tick (qp_resident_box_front4_kernel: robot variables only)
constexpr bool qp_resident_ok(const ShapeDesc& sd) { return qp_front4_ok(sd) && sd.n_x == 0; }

// ---- the launchers' signatures ---------------------------------------------------------------------------------
// The ahead-of-time table (clik_qp_shapes.hip) holds launch_qp_static / launch_qp_rollout_static; the objects compiled
// at run time (casclik_amd/jit.py) export the same launchers and the value-specialised ones (clik_qp_static.hpp).
// t_inst: null (tk serves the whole batch) or one time-slot record per instance ([B][2 * n_tslots], device)
typedef hipError_t (*qp_static_fn)(const void*, const TickArgs&, long long, const double*, const double*,
                                   const double*, double*, double*, double*, int32_t*, int32_t*, int, hipStream_t,
                                   const double*);
// stages: controller evaluations per tick (1 explicit Euler, 4 classical Runge-Kutta)
typedef hipError_t (*qp_static_rollout_fn)(const void*, const double*, int, double, double, long long, double*,
                                           const double*, double*, double*, int32_t*, double*, double*, hipStream_t,
                                           int);
// clik_jit_qp_solve: launch_qp_static with the tick's arguments by address
typedef hipError_t (*qp_jit_fn)(const void*, const TickArgs*, long long, const double*, const double*,
                                const double*, double*, double*, double*, int32_t*, int32_t*, int, hipStream_t,
                                const double*);
// clik_jit_qp_value_solve / _rollout / _resident: the skill's numbers compiled in, no image argument
typedef hipError_t (*qp_value_fn)(const TickArgs*, long long, const double*, const double*, const double*,
                                  double*, double*, double*, int32_t*, int32_t*, int, hipStream_t);
typedef hipError_t (*qp_value_rollout_fn)(const double*, int, double, double, long long, double*, const double*,
                                          double*, double*, int32_t*, double*, double*, hipStream_t, int);
typedef hipError_t (*qp_value_resident_fn)(const TickArgs*, long long, const double*, const double*, double*, double*,
                                           int32_t*, void*, unsigned*, int, unsigned long long, hipStream_t);

// ---- the value-specialised tick ----------------------------------------------------------------------------------
// The switches of the value-specialised launcher, read once per loaded object.
// CLIK_QP_FOLIO: unset or starting with '1' = the four-waves-per-64-instances kernel for cold ticks of small batches,
// anything else (the empty string too) = never.  CLIK_QP_FOLIO_SAME=1 (measuring switch): those four waves all start
// like the lone-wave kernel.
struct QpEnv {
    bool folio;
    bool folio_same;
};
inline const QpEnv& qp_env()
{
    static const QpEnv env = []() {
        const char* f = getenv("CLIK_QP_FOLIO");
        const char* s = getenv("CLIK_QP_FOLIO_SAME");
        return QpEnv{!f || f[0] == '1', s && s[0] == '1'};
    }();
    return env;
}

// compute units of the current device, 0 when it cannot be asked (per CURRENT device: a process may drive several, or a
// partition of one)
inline int current_device_cus()
{
    static int cached[16] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 16 && cached[dev] > 0) return cached[dev];
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (dev >= 0 && dev < 16) cached[dev] = cus;
    return cus;
}

// Which value-specialised QP kernel serves a tick of B instances: the one with the LDS work area outside the box
// family; in it, the four-waves-per-64-instances kernel (FOLIO) for cold ticks of up to ONE block per CU (16384
// instances on 256 CUs) - measured per tick against the lone-wave kernel: 10.2 / 11.0 us at 1024 instances, 10.4 / 12.0
// at 4096, 11.0 / 12.0 at 8192, 11.2 / 12.1 at 12288, the same at 256 and 2048, 11.0 - 11.1 / 11.3 at 16384 (four
// identical waves cost 12.2 - 12.5 us there - slower waves, not a slower dispatch: tools/stamp_folio.py - and the
// different starts win 1.3 - 1.6 back, 0.4 of it through the second look half-way through a pass; six input seeds: -7 %
// on average, every one a gain; profiles/r4_qp_wave_portfolio.txt); the lone-wave kernel otherwise.  The launcher
// (launch_qp_static_values) and the label (clik_qp_kernel_variant, through qp_select) both ask this.
enum QpValueKernel { QPV_GENERAL = 0, QPV_LONE, QPV_FOLIO };
constexpr QpValueKernel qp_value_select(bool box, bool folio_on, long long B, bool hot, int cus)
{
    if (!box) return QPV_GENERAL;
    if (folio_on && !hot && (B + WAVE - 1) / WAVE <= (long long)cus) return QPV_FOLIO;
    return QPV_LONE;
}

// ---- the choice ------------------------------------------------------------------------------------------------
// A handle's switches: clik_qp_create fills them once, clik_qp_attach_value_kernel sets values_attached.
struct QpPolicy {
    bool aot;               // the ahead-of-time table may serve (CLIK_FORCE_DYNAMIC=1 / CLIK_NO_AOT=1: not)
    bool values_attached;   // a value-specialised tick is attached
    bool folio;             // qp_env().folio
    int  cus;               // compute units of the device the handle was created on (host-only handle: 0)
};

// What else a handle has, as far as the choice goes.
struct QpKernels {
    bool aot;               // the ahead-of-time table serves the shape
    bool jit_solve;         // a shape-specialised tick compiled at run time is attached ...
    bool jit_rollout;       // ... and its rollout
    bool value_rollout;     // the value-specialised rollout is attached (box family)
    int  dyn_width;         // rows per constraint of the built-in (dynamic) variant, 0: none fits the skill
    bool generated;         // some constraint has code-generated rows or attributes
    bool wide;              // some constraint has more than CLIK_DYN_MAX_M rows
};

// the kernels that serve a QP entry point; "none" and "needs_instance" are refusals
enum class QpKernel : int { value_folio, value, jit, aot, dynamic, none, needs_instance };
// ... and what clik_qp_kernel_variant reports behind clik_qp_kernel_name for them (bench.py and the tests read it)
constexpr const char* kQpVariantName[] = {"/v/folio4", "/v", "", "", "", "", ""};

// tick: clik_qp_solve_batch(_hot); tick_t: per-instance time (clik_qp_solve_batch_t); rollout: clik_qp_rollout_batch_*;
// data: clik_qp_data_batch (the built-in kernel's H / A / bounds)
enum class QpOp : int { tick, tick_t, rollout, data };

// The kernel that serves an entry point for B instances (hot: a hot-started tick).  The label, the attach gates and
// every QP entry point read it.
constexpr QpKernel qp_select(const ShapeDesc& sd, const QpPolicy& p, const QpKernels& k, long long B, bool hot, QpOp op)
{
    // generated constraint code, and constraints wider than the built-in variant, exist only in an instantiated kernel
    const bool needs_instance = k.generated || (k.wide && k.dyn_width <= CLIK_DYN_MAX_M);
    const QpKernel dynamic = k.dyn_width > 0 ? QpKernel::dynamic : QpKernel::none;
    switch (op) {
    case QpOp::data:
        return needs_instance ? QpKernel::needs_instance : dynamic;
    case QpOp::rollout:
        if (!k.jit_rollout && !k.aot) return QpKernel::none;
        return k.value_rollout ? QpKernel::value : k.jit_rollout ? QpKernel::jit : QpKernel::aot;
    default:
        if (!k.jit_solve && !k.aot) {
            if (needs_instance) return QpKernel::needs_instance;
            return op == QpOp::tick ? dynamic : QpKernel::none;     // (per-instance time: shape-specialised only)
        }
        if (op == QpOp::tick && p.values_attached)
            return qp_value_select(CLIK_QP_BOX_OK(sd), p.folio, B, hot, p.cus) == QPV_FOLIO ? QpKernel::value_folio
                                                                                            : QpKernel::value;
        return k.jit_solve ? QpKernel::jit : QpKernel::aot;
    }
}

// a shape-specialised kernel (compiled ahead of time or at run time) serves the skill's ticks
constexpr bool qp_shape_kernel(QpKernel k) { return k == QpKernel::jit || k == QpKernel::aot; }

}  // namespace clik
