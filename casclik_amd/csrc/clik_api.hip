// C ABI (include/clik.h) of the MI355X batched CLIK hot path: handle
// management, descriptor validation, mode table, kernel dispatch.
//
// Every entry point replaces a piece of the reference's controller setup/solve:
//   clik_pinv_create       <- PseudoInverseController.setup_problem_functions
//                             (pseudo_inverse.py:453-483) + create_activation_map (:107-130)
//   clik_pinv_solve_batch  <- PseudoInverseController.solve (:512-556)
//   clik_qp_create         <- ReactiveQPController.setup_problem_functions / setup_solver
//                             (reactive_qp.py:248-298)
//   clik_qp_solve_batch    <- ReactiveQPController.solve (:461-528)
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "clik_device.hpp"
#include "clik_pinv_select.hpp"
#include "clik_qp_select.hpp"
#include "clik_workspace.hpp"
#include "clik_launch.hpp"

using clik::DevSkill;
using clik::TickArgs;
using clik::WarmArgs;

typedef hipError_t (*clik_jit_solve_fn)(const clik::LaunchArgs*, const TickArgs*, long long, const double*,
                                        const double*, const double*, double*, double*, int32_t*, hipStream_t);
typedef hipError_t (*clik_jit_rollout_fn)(const clik::LaunchArgs*, const double*, int, double, double, long long,
                                          double*, const double*, double*, int32_t*, hipStream_t);

// clik_jit_time_terms (casclik_amd/jit.py, clik_time.hpp): times [n] (device) -> time-slot records [n * stages][2 * n_tslots]
typedef hipError_t (*clik_time_fn)(const double*, long long, int, double, double*, hipStream_t);

// clik_jit_constraint_values (casclik_amd/jit.py, clik_monitor.hpp): skill image, n_rec, B, time-term table and its two
// strides, q, x, y and its record stride, e, J, et (all device)
typedef hipError_t (*clik_monitor_fn)(const void*, long long, long long, const double*, long long, long long,
                                      const double*, const double*, const double*, long long, double*, double*, double*,
                                      hipStream_t);

// clik_jit_constraint_summary / clik_jit_summary_work_bytes (casclik_amd/jit.py, clik_summary.hpp): as clik_monitor_fn up
// to y_stride, then tol, the work area and its size, the seven outputs (all device)
typedef hipError_t (*clik_summary_fn)(const void*, long long, long long, const double*, long long, long long,
                                      const double*, const double*, const double*, long long, const double*, void*,
                                      unsigned long long, double*, int32_t*, double*, double*, double*, int32_t*, int32_t*,
                                      hipStream_t);
typedef unsigned long long (*clik_summary_work_fn)(long long, long long);

// clik_jit_rollout_sum (casclik_amd/jit.py, clik_rollout_summary.hpp): the arguments of clik_jit_rollout_rec, then tol and
// the seven outputs of the summary (all device)
typedef hipError_t (*clik_rollsum_fn)(const clik::LaunchArgs*, const double*, int, double, double, long long, double*,
                                      const double*, double*, int32_t*, hipStream_t, const double*, double*, int32_t*,
                                      double*, double*, double*, int32_t*, int32_t*);

// clik_jit_converge (casclik_amd/jit.py, clik_converge.hpp): one TickArgs record, B, max_ticks, dt, max_speed, min_step,
// q, y, dq, mode, the stream, then tol, ticks, stop_status, residual (all device)
typedef hipError_t (*clik_converge_fn)(const clik::LaunchArgs*, const TickArgs*, long long, int, double, double, double,
                                       double*, const double*, double*, int32_t*, hipStream_t, const double*, int32_t*,
                                       int32_t*, double*);

typedef hipError_t (*clik_jit_value_fn)(const clik::LaunchArgs*, const TickArgs*, long long, const double*,
                                        const double*, double*, int32_t*, hipStream_t);

// What both handles hold: the skill (host copy, device copy, warm-up ranges, image on the device) and the kernels that
// do not depend on the controller.  The handle owns its device memory: `delete h` releases it.
struct clik_handle {
    DevSkill  host = {};
    DevSkill* dev = nullptr;        // null: a host-only handle (clik_*_create_host)
    clik::WarmArgs warm = {};
    void*     d_img = nullptr;      // shape-specialised kernels: device copy of the skill image (QP: + the QP options)
    char      jit_name[64] = "";
    clik_time_fn time_fn = nullptr;         // the skill's time slots as device code (clik_*_attach_time_kernel)
    clik_monitor_fn monitor_fn = nullptr;   // e, J, d e / d t of the constraints over a trajectory (clik_*_attach_monitor_kernel)
    clik_summary_fn summary_fn = nullptr;   // per-instance summaries of them (clik_*_attach_summary_kernel)
    clik_summary_work_fn summary_work_fn = nullptr;
    clik_handle() = default;
    clik_handle(const clik_handle&) = delete;
    clik_handle& operator=(const clik_handle&) = delete;
    ~clik_handle()
    {
        if (d_img) (void)hipFree(d_img);
        if (dev) (void)hipFree(dev);
    }
};

struct clik_pinv : clik_handle {
    clik::PinvPolicy policy = {};   // the switches pinv_select reads
    // shape-specialised kernel attached at run time (clik_pinv_attach_kernel)
    clik_jit_solve_fn   jit_solve = nullptr;
    clik_jit_rollout_fn jit_rollout = nullptr;
    int       kernel = -1;          // index into the kernel table (static shape or dynamic)
    // team kernel with this skill's numbers compiled in (clik_pinv_attach_value_kernel), used for the batches the
    // image-reading team kernel would serve
    clik_jit_value_fn   val_solve = nullptr;
    clik_jit_rollout_fn val_rollout = nullptr;
    // ... and its resident form (clik_pinv_attach_resident_kernel)
    hipError_t (*val_resident)(const TickArgs*, long long, const double*, const double*, double*, int32_t*, void*,
                               unsigned*, int, unsigned long long, hipStream_t) = nullptr;
    // the recording / per-tick-target rollouts (clik_pinv_attach_rec_kernel): image-reading and value-specialised
    clik_jit_rollout_fn rec_rollout = nullptr;
    clik_jit_rollout_fn val_rec_rollout = nullptr;
    // the rollout that summarises the constraint values while it runs (clik_pinv_attach_rollout_summary_kernel)
    clik_rollsum_fn rollsum_fn = nullptr;
    // the rollout that runs until each instance has converged (clik_pinv_attach_converge_kernel)
    clik_converge_fn converge_fn = nullptr;
};

// clik_jit_qp_rollout_rec / clik_jit_qp_value_rollout_rec: the rollouts' arguments and the RollRec
typedef hipError_t (*clik_qp_rec_fn)(const void*, const double*, int, double, double, long long, double*, const double*,
                                     double*, double*, int32_t*, double*, double*, hipStream_t, int, const clik::RollRec*);
typedef hipError_t (*clik_qp_value_rec_fn)(const double*, int, double, double, long long, double*, const double*, double*,
                                           double*, int32_t*, double*, double*, hipStream_t, int, const clik::RollRec*);
// clik_jit_qp_rollout_sum: the arguments of clik_jit_qp_rollout_rec, then tol and the seven outputs of the summary
typedef hipError_t (*clik_qp_rollsum_fn)(const void*, const double*, int, double, double, long long, double*, const double*,
                                         double*, double*, int32_t*, double*, double*, hipStream_t, int, const clik::RollRec*,
                                         const double*, double*, int32_t*, double*, double*, double*, int32_t*, int32_t*);

// clik_jit_qp_converge: the skill image, one TickArgs record, B, max_ticks, dt, max_speed, min_step, q, y, dq, slack,
// status, x, dx, the stream, then tol, ticks, stop_status, residual
typedef hipError_t (*clik_qp_converge_fn)(const void*, const TickArgs*, long long, int, double, double, double, double*,
                                          const double*, double*, double*, int32_t*, double*, double*, hipStream_t,
                                          const double*, int32_t*, int32_t*, double*);

struct clik_qp : clik_handle {
    int       variant = -1;     // dynamic kernel variant (qp_data and the fallback use it); -1: the skill only fits
                                // the shape-specialised kernels
    int       static_k = -1;    // AOT shape-specialised kernel, -1 none
    clik::QpPolicy policy = {}; // the switches qp_select reads
    clik::qp_jit_fn jit_solve = nullptr;
    clik::qp_static_rollout_fn jit_rollout = nullptr;
    clik::qp_value_fn val_solve = nullptr;     // per-tick kernel with this skill's numbers and QP options compiled in
    clik::qp_value_rollout_fn val_rollout = nullptr;   // ... and its on-device rollout (box family), or null
    clik::qp_value_resident_fn val_resident = nullptr; // ... and its resident form (clik_qp_attach_resident_kernel), or null
    // the recording / per-tick-target rollouts (clik_qp_attach_rec_kernel): image-reading and value-specialised (box)
    clik_qp_rec_fn rec_rollout = nullptr;
    clik_qp_value_rec_fn val_rec_rollout = nullptr;
    clik_qp_rollsum_fn rollsum_fn = nullptr; // the rollout that summarises them (clik_qp_attach_rollout_summary_kernel)
    clik_qp_converge_fn converge_fn = nullptr; // the rollout that runs to convergence (clik_qp_attach_converge_kernel)
    // work area of the global-workspace kernels (clik_workspace.hpp): belongs to this handle, released with it
    std::unique_ptr<clik::GwsOwner> gws;
    // (runs before the base frees dev and d_img; the three allocations are independent, so the order does not matter)
    ~clik_qp()
    {
        if (gws) gws->release();
    }
};

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int hipfail(hipError_t e, const char* what)
{
    return fail(CLIK_EHIP, "%s: %s", what, hipGetErrorString(e));
}

extern "C" const char* clik_last_error(void) { return g_err; }
extern "C" int32_t clik_abi_version(void) { return CLIK_ABI_VERSION; }

static int popcount32(unsigned v)
{
    int c = 0;
    while (v) { c += v & 1u; v >>= 1; }
    return c;
}

// Structural validation shared by both controllers; fills the derived fields.  *used_rows (may be null): the number of
// affine rows the constraints use, for the warm-up ranges.
static int validate_and_derive(const clik_skill_desc* d, DevSkill* S, int* used_rows = nullptr)
{
    if (!d) return fail(CLIK_EINVAL, "null skill descriptor");
    if (d->abi_version != CLIK_ABI_VERSION)
        return fail(CLIK_EINVAL, "descriptor ABI version %d, library %d", d->abi_version, CLIK_ABI_VERSION);
    const int n = d->n_q + d->n_x;
    if (d->n_q < 1 || d->n_x < 0 || n > CLIK_MAX_DOF)
        return fail(CLIK_EUNSUPPORTED, "n_robot_var + n_virtual_var = %d outside [1, %d]", n, CLIK_MAX_DOF);
    if (d->n_y < 0) return fail(CLIK_EINVAL, "negative n_y");
    if (d->n_joints < 0 || d->n_joints > CLIK_MAX_JOINTS)
        return fail(CLIK_EUNSUPPORTED, "chain has %d joints (limit %d)", d->n_joints, CLIK_MAX_JOINTS);
    if (d->n_tasks < 0 || d->n_tasks > CLIK_MAX_TASKS)
        return fail(CLIK_EUNSUPPORTED, "%d constraints (limit %d)", d->n_tasks, CLIK_MAX_TASKS);
    if (d->n_rows < 0 || d->n_rows > CLIK_MAX_ROWS) return fail(CLIK_EUNSUPPORTED, "too many affine rows");
    if (d->n_tslots < 0 || d->n_tslots > CLIK_MAX_TSLOTS) return fail(CLIK_EUNSUPPORTED, "too many time slots");
    if (d->quat_src < 0 || d->quat_src > 2) return fail(CLIK_EINVAL, "bad quat_src");
    if (d->quat_src == 2)
        for (int i = 0; i < 4; ++i)
            if (d->quat_yi[i] < 0 || d->quat_yi[i] >= d->n_y)
                return fail(CLIK_EINVAL, "orientation target index outside input_var");
    memset(S, 0, sizeof(*S));
    S->d = *d;
    S->n = n;
    bool any_fk = false, any_o = false;
    for (int j = 0; j < d->n_joints; ++j) {
        const clik_joint& jt = d->joints[j];
        int jf = 0;
        static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        bool r_ident = true;
        for (int k = 0; k < 9; ++k) r_ident = r_ident && (jt.R[k] == I3[k]);    // -0.0 == 0.0
        if (r_ident) jf |= 1;
        if (jt.p[0] == 0.0 && jt.p[1] == 0.0 && jt.p[2] == 0.0) jf |= 2;
        if (jt.type != CLIK_JOINT_FIXED)
            for (int k = 0; k < 3; ++k) {
                const double a = jt.axis[k], b = jt.axis[(k + 1) % 3], c = jt.axis[(k + 2) % 3];
                if (b == 0.0 && c == 0.0 && (a == 1.0 || a == -1.0)) jf |= ((k + 1) | (a < 0 ? 4 : 0)) << 4;
            }
        S->jflags[j] = jf;
        S->shape.jtype[j] = jt.type;
        S->shape.jq[j] = (jt.type == CLIK_JOINT_FIXED) ? -1 : jt.q_index;
        S->shape.jflags[j] = jf;
        if (jt.type == CLIK_JOINT_FIXED) continue;
        if (jt.type != CLIK_JOINT_REVOLUTE && jt.type != CLIK_JOINT_PRISMATIC)
            return fail(CLIK_EINVAL, "joint %d: unknown type %d", j, jt.type);
        if (jt.q_index < 0 || jt.q_index >= n) return fail(CLIK_EINVAL, "joint %d: q_index out of range", j);
        if (S->used_mask & (1u << jt.q_index))
            return fail(CLIK_EUNSUPPORTED, "state variable %d drives two joints", jt.q_index);
        S->used_mask |= 1u << jt.q_index;
        if (jt.type == CLIK_JOINT_REVOLUTE) S->rev_mask |= 1u << jt.q_index;
    }
    int n_sets = 0, n_slack = 0, n_rows_qp = 0;
    for (int ti = 0; ti < d->n_tasks; ++ti) {
        const clik_task& t = d->tasks[ti];
        if (t.cls < CLIK_CLS_EQ || t.cls > CLIK_CLS_VELSET) return fail(CLIK_EINVAL, "task %d: bad class", ti);
        if (t.attr_ext & ~(CLIK_ATTR_GAIN | CLIK_ATTR_SET_MIN | CLIK_ATTR_SET_MAX | CLIK_ATTR_TARGET))
            return fail(CLIK_EINVAL, "task %d: bad attr_ext", ti);
        if (t.attr_ext != 0 && ti >= clik::SHAPE_MAX_TASKS)
            return fail(CLIK_EUNSUPPORTED, "task %d: attributes given as expressions need a shape-specialised kernel "
                                           "(at most %d constraints)", ti, clik::SHAPE_MAX_TASKS);
        if (t.m < 1 || t.m > CLIK_MAX_M)
            return fail(CLIK_EUNSUPPORTED, "task %d: %d rows (limit %d)", ti, t.m, CLIK_MAX_M);
        for (int i = 0; i < t.m; ++i) {
            const int r0 = t.out_row0[i];
            const int nr = (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 1;
            if (t.out_kind[i] != CLIK_OUT_AFFINE && t.out_kind[i] != CLIK_OUT_NORM2 &&
                t.out_kind[i] != CLIK_OUT_EXTERN)
                return fail(CLIK_EINVAL, "task %d row %d: bad out_kind", ti, i);
            if ((t.out_kind[i] == CLIK_OUT_EXTERN) != (t.out_kind[0] == CLIK_OUT_EXTERN))
                return fail(CLIK_EINVAL, "task %d: EXTERN outputs cannot be mixed with table rows", ti);
            if (t.out_kind[i] == CLIK_OUT_EXTERN && ti >= clik::SHAPE_MAX_TASKS)
                return fail(CLIK_EUNSUPPORTED, "code-generated constraints need a shape-specialised kernel "
                                               "(at most %d constraints)", clik::SHAPE_MAX_TASKS);
            if (nr < 0 || r0 < 0 || r0 + nr > d->n_rows) return fail(CLIK_EINVAL, "task %d row %d: row range", ti, i);
            for (int k = r0; k < r0 + nr; ++k) {
                const clik_row& r = d->rows[k];
                if (r.flags & (CLIK_ROW_HAS_P | CLIK_ROW_HAS_R | CLIK_ROW_HAS_O)) any_fk = true;
                if (r.flags & CLIK_ROW_HAS_O) any_o = true;
                if ((r.flags & CLIK_ROW_HAS_T) && (r.t_slot < 0 || r.t_slot >= d->n_tslots))
                    return fail(CLIK_EINVAL, "row %d: t_slot out of range", k);
                if (r.n_y < 0 || r.n_y > CLIK_MAX_YTERMS) return fail(CLIK_EINVAL, "row %d: n_y", k);
                for (int q = 0; q < r.n_y; ++q)
                    if (r.yi[q] < 0 || r.yi[q] >= d->n_y) return fail(CLIK_EINVAL, "row %d: input index", k);
            }
        }
        if (t.cls == CLIK_CLS_SET) ++n_sets;
        if (t.soft) n_slack += t.m;
        n_rows_qp += t.m;
    }
    // per-task feature flags, constant-Jacobian detection, shape descriptor
    S->shape.n = n;
    S->shape.n_y = d->n_y;
    S->shape.n_x = d->n_x;
    S->shape.nj = d->n_joints;
    S->shape.n_tasks = d->n_tasks;
    S->shape.all_affine = 1;
    int last_row = 0;
    for (int ti = 0; ti < d->n_tasks; ++ti) {
        const clik_task& t = d->tasks[ti];
        int fl = 0, affine = 1;
        for (int i = 0; i < t.m; ++i) {
            const int nr = (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 1;
            if (t.out_kind[i] != CLIK_OUT_AFFINE) affine = 0;
            for (int k = t.out_row0[i]; k < t.out_row0[i] + nr; ++k) fl |= d->rows[k].flags;
            if (t.out_row0[i] + nr > last_row) last_row = t.out_row0[i] + nr;
        }
        S->task_flags[ti] = fl;
        S->task_const_j[ti] =
            (affine && !(fl & (CLIK_ROW_HAS_P | CLIK_ROW_HAS_R | CLIK_ROW_HAS_O))) ? 1 : 0;
        if (!affine) S->shape.all_affine = 0;
        if (ti < clik::SHAPE_MAX_TASKS) {
            S->shape.cls[ti] = t.cls;
            S->shape.m[ti] = t.m;
            // time terms do not change the code path of a row: drop the flag from the shape
            S->shape.flags[ti] = fl & ~CLIK_ROW_HAS_T;
            S->shape.const_j[ti] = S->task_const_j[ti];
            S->shape.gain_matrix[ti] = t.gain_is_matrix ? 1 : 0;
            S->shape.ext[ti] = ((t.out_kind[0] == CLIK_OUT_EXTERN) ? 1 : 0) | ((t.attr_ext & 15) << 1);
            int nyt = 0;
            for (int i = 0; i < t.m; ++i) {
                const int nrw = (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 1;
                for (int k = 0; k < nrw; ++k)
                    if (d->rows[t.out_row0[i] + k].n_y > nyt) nyt = d->rows[t.out_row0[i] + k].n_y;
            }
            S->shape.ny_terms[ti] = nyt;
            S->shape.has_t[ti] = (fl & CLIK_ROW_HAS_T) ? 1 : 0;
            // joint-space task: rows are distinct unit vectors (clik_device.hpp, ShapeDesc::ucol)
            bool unit = S->task_const_j[ti] != 0 && t.m > 0 && t.m <= CLIK_MAX_M;
            int cols[CLIK_MAX_M] = {0};
            unsigned seen = 0;
            for (int i = 0; i < t.m && unit; ++i) {
                const clik_row& r = d->rows[t.out_row0[i]];
                int col = -1;
                for (int j = 0; j < n; ++j) {
                    if (r.a[j] == 0.0) continue;
                    if (r.a[j] != 1.0 || col >= 0) { unit = false; break; }
                    col = j;
                }
                if (col < 0 || (seen >> col) & 1u) unit = false;
                else { seen |= 1u << col; cols[i] = col + 1; }
            }
            for (int i = 0; i < CLIK_MAX_M; ++i) S->shape.ucol[ti][i] = (unit && i < t.m) ? cols[i] : 0;
        }
        if (fl & CLIK_ROW_HAS_T) S->shape.all_affine = S->shape.all_affine;  // (time slots are run-time data)
    }
    // feature-coefficient patterns of the rows in task order (what the static kernels index:
    // rows of static shapes are contiguous); skills with other row layouts never match a static shape
    for (int r = 0; r < clik::SHAPE_MAX_ROWS; ++r) S->shape.row_nz[r] = S->shape.row_one[r] = 0u;
    {
        int r = 0;
        for (int ti = 0; ti < d->n_tasks && ti < clik::SHAPE_MAX_TASKS; ++ti) {
            const clik_task& t = d->tasks[ti];
            for (int i = 0; i < t.m; ++i) {
                const int nrw = (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 1;
                S->shape.out_nrows[ti][i] = (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 0;
                for (int k2 = 0; k2 < nrw; ++k2, ++r) {
                    if (r >= clik::SHAPE_MAX_ROWS) continue;
                    const clik_row& row = d->rows[t.out_row0[i] + k2];
                    unsigned nz = 0u, one = 0u;
                    auto mark = [&](double v, int bit) {
                        if (v != 0.0) nz |= 1u << bit;
                        if (v == 1.0) one |= 1u << bit;
                    };
                    if (row.flags & CLIK_ROW_HAS_P) for (int k = 0; k < 3; ++k) mark(row.b[k], k);
                    if (row.flags & CLIK_ROW_HAS_R) for (int k = 0; k < 9; ++k) mark(row.g[k], 3 + k);
                    if (row.flags & CLIK_ROW_HAS_O) for (int k = 0; k < 3; ++k) mark(row.h[k], 12 + k);
                    S->shape.row_nz[r] = nz;
                    S->shape.row_one[r] = one;
                }
            }
        }
    }
    S->shape.uses_fk = any_fk ? 1 : 0;
    S->shape.quat_src = any_o ? d->quat_src : 0;
    if (used_rows) *used_rows = last_row;
    if (any_fk && d->n_joints == 0) return fail(CLIK_EINVAL, "rows use the tool frame but the chain is empty");
    if (any_o && d->quat_src == 0) return fail(CLIK_EINVAL, "rows use the orientation error but no target is set");
    S->d.uses_fk = any_fk ? 1 : 0;
    S->n_sets = n_sets;
    S->n_slack = n_slack;
    S->n_qp_rows = n_rows_qp;
    S->n_qp_vars = n + n_slack;
    return CLIK_OK;
}

// dense solve A X = B (A k x k, B k x c, row-major), partial pivoting; host only
static bool host_solve(int k, int c, double* A, double* B)
{
    for (int col = 0; col < k; ++col) {
        int piv = col;
        for (int r = col + 1; r < k; ++r)
            if (std::fabs(A[r * k + col]) > std::fabs(A[piv * k + col])) piv = r;
        if (A[piv * k + col] == 0.0) return false;
        if (piv != col) {
            for (int j = 0; j < k; ++j) std::swap(A[col * k + j], A[piv * k + j]);
            for (int j = 0; j < c; ++j) std::swap(B[col * c + j], B[piv * c + j]);
        }
        for (int r = col + 1; r < k; ++r) {
            const double f = A[r * k + col] / A[col * k + col];
            for (int j = col; j < k; ++j) A[r * k + j] -= f * A[col * k + j];
            for (int j = 0; j < c; ++j) B[r * c + j] -= f * B[col * c + j];
        }
    }
    for (int col = k - 1; col >= 0; --col)
        for (int j = 0; j < c; ++j) {
            double s = B[col * c + j];
            for (int r = col + 1; r < k; ++r) s -= A[col * k + r] * B[r * c + j];
            B[col * c + j] = s / A[col * k + col];
        }
    return true;
}

// P (n x m, ld CLIK_MAX_M) = pinv(J) with the controller's method
// (pseudo_inverse.py:92-105) for a state-independent Jacobian J (m x n)
static bool host_const_pinv(const clik_pinv_opts& o, int m, int n, const double* J, double* P)
{
    const bool standard = o.pinv_method == CLIK_PINV_STANDARD;
    const double lam = standard ? 0.0 : o.damping_factor;
    const bool wide = standard ? (m < n) : (n >= m);
    double A[CLIK_MAX_M * CLIK_MAX_M], X[CLIK_MAX_M * CLIK_MAX_M];
    if (wide) {
        for (int i = 0; i < m; ++i)
            for (int k = 0; k < m; ++k) {
                double sacc = (i == k) ? lam : 0.0;
                for (int j = 0; j < n; ++j) sacc += J[i * n + j] * J[k * n + j];
                A[i * m + k] = sacc;
            }
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < n; ++j) X[i * n + j] = J[i * n + j];
        if (!host_solve(m, n, A, X)) return false;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < m; ++i) P[j * CLIK_MAX_M + i] = X[i * n + j];
    } else {
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) {
                double sacc = (a == b) ? lam : 0.0;
                for (int i = 0; i < m; ++i) sacc += J[i * n + a] * J[i * n + b];
                A[a * n + b] = sacc;
            }
        for (int a = 0; a < n; ++a)
            for (int i = 0; i < m; ++i) X[a * m + i] = J[i * n + a];
        if (!host_solve(n, m, A, X)) return false;
        for (int a = 0; a < n; ++a)
            for (int i = 0; i < m; ++i) P[a * CLIK_MAX_M + i] = X[a * m + i];
    }
    return true;
}

// Compact skill image for the shape-specialised kernels; layout =
// clik::SkillImage<nj, nt, nr> (clik_device.hpp), padded to a multiple of 1 KiB.
// Static shapes require the rows contiguous in task / output order.
static bool build_skill_image(const DevSkill& S, std::vector<char>& out, size_t* image_bytes = nullptr,
                              size_t extra = 0)
{
    const int nj = S.d.n_joints, nt = S.d.n_tasks;
    int nr = 0;
    for (int ti = 0; ti < nt; ++ti) {
        const clik_task& t = S.d.tasks[ti];
        for (int i = 0; i < t.m; ++i) {
            // rows in task order, output order; a 2-norm output owns a group of consecutive rows
            if (t.out_row0[i] != nr) return false;
            nr += (t.out_kind[i] == CLIK_OUT_NORM2) ? t.out_nrows[i] : 1;
        }
    }
    if (nr > clik::SHAPE_MAX_ROWS) return false;
    const size_t o_j = 0;
    const size_t o_t = o_j + sizeof(clik_joint) * (size_t)(nj > 0 ? nj : 1);
    const size_t o_r = o_t + sizeof(clik_task) * (size_t)nt;
    const size_t o_c = o_r + sizeof(clik_row) * (size_t)nr;
    const size_t o_g = o_c + sizeof(double) * CLIK_MAX_DOF * CLIK_MAX_M * (size_t)nt;
    constexpr size_t GT = CLIK_MAX_DOF * (CLIK_MAX_DOF + 1) / 2;
    const size_t o_tail = o_g + sizeof(double) * GT * (size_t)nt;
    const size_t total = o_tail + sizeof(double) * 5 + sizeof(int32_t) * 6;
    if (image_bytes) *image_bytes = total;
    out.assign((((total + 15) & ~(size_t)15) + extra + 1023) / 1024 * 1024, 0);
    memcpy(&out[o_j], S.d.joints, sizeof(clik_joint) * (size_t)nj);
    memcpy(&out[o_t], S.d.tasks, sizeof(clik_task) * (size_t)nt);
    memcpy(&out[o_r], S.d.rows, sizeof(clik_row) * (size_t)nr);
    for (int ti = 0; ti < nt; ++ti)
        memcpy(&out[o_c + sizeof(double) * CLIK_MAX_DOF * CLIK_MAX_M * (size_t)ti], S.cpinv[ti],
               sizeof(double) * CLIK_MAX_DOF * CLIK_MAX_M);
    // J^T J of the constant-Jacobian tasks, packed lower triangle tri(a,b) = a(a+1)/2 + b
    for (int ti = 0; ti < nt; ++ti) {
        if (!S.task_const_j[ti]) continue;
        const clik_task& t = S.d.tasks[ti];
        double* g = reinterpret_cast<double*>(&out[o_g + sizeof(double) * GT * (size_t)ti]);
        for (int a = 0; a < S.n; ++a)
            for (int b = 0; b <= a; ++b) {
                double acc = 0.0;
                for (int i = 0; i < t.m; ++i)
                    acc += S.d.rows[t.out_row0[i]].a[a] * S.d.rows[t.out_row0[i]].a[b];
                g[a * (a + 1) / 2 + b] = acc;
            }
    }
    // unused input_var terms must read index 0 with coefficient 0
    for (int r = 0; r < nr; ++r) {
        clik_row* row = reinterpret_cast<clik_row*>(&out[o_r + sizeof(clik_row) * (size_t)r]);
        for (int k = row->n_y; k < CLIK_MAX_YTERMS; ++k) { row->yc[k] = 0.0; row->yi[k] = 0; }
    }
    double tail_d[5] = {S.po.pinv_method == CLIK_PINV_STANDARD ? 0.0 : S.po.damping_factor,
                        S.d.quat[0], S.d.quat[1], S.d.quat[2], S.d.quat[3]};
    int32_t tail_i[6] = {S.d.quat_yi[0], S.d.quat_yi[1], S.d.quat_yi[2], S.d.quat_yi[3], S.d.n_tslots, 0};
    memcpy(&out[o_tail], tail_d, sizeof(tail_d));
    memcpy(&out[o_tail + sizeof(tail_d)], tail_i, sizeof(tail_i));
    return true;
}

// scalar-cache warm-up ranges (clik_device.hpp, warm_descriptor): the used
// prefixes of the descriptor arrays and the derived tables
static void compute_warm(const DevSkill& S, int used_rows, clik::WarmArgs& w)
{
    auto lo = [](size_t off) { return (int32_t)(off & ~(size_t)63); };
    auto hi = [](size_t off) { return (int32_t)((off + 63) & ~(size_t)63); };
    const size_t o_d = offsetof(DevSkill, d);
    w.off[0] = lo(o_d);
    w.end[0] = hi(o_d + offsetof(clik_skill_desc, joints) + (size_t)S.d.n_joints * sizeof(clik_joint));
    w.off[1] = lo(o_d + offsetof(clik_skill_desc, tasks));
    w.end[1] = hi(o_d + offsetof(clik_skill_desc, tasks) + (size_t)S.d.n_tasks * sizeof(clik_task));
    w.off[2] = lo(o_d + offsetof(clik_skill_desc, rows));
    w.end[2] = hi(o_d + offsetof(clik_skill_desc, rows) + (size_t)used_rows * sizeof(clik_row));
    w.off[3] = lo(offsetof(DevSkill, shape));
    w.end[3] = hi(offsetof(DevSkill, cpinv) + (size_t)S.d.n_tasks * sizeof(S.cpinv[0]));
    w.off[4] = lo(offsetof(DevSkill, po));
    w.end[4] = hi(sizeof(DevSkill));
    w.token_off = (int32_t)offsetof(DevSkill, zero_token);
}

static void finish_pinv_shape(DevSkill& S, const clik_pinv_opts* opts)
{
    S.po = *opts;
    S.shape.feedforward = opts->feedforward ? 1 : 0;
    S.shape.multidim = opts->multidim_sets ? 1 : 0;
    S.shape.conv_last = opts->converge_final_set_to_max ? 1 : 0;
    S.shape.standard = opts->pinv_method == CLIK_PINV_STANDARD ? 1 : 0;
    S.shape.qp = 0;
    for (int ti = 0; ti < clik::SHAPE_MAX_TASKS; ++ti) S.shape.soft[ti] = 0;
}

// shape of a ReactiveQPController: no pinv options, per-task soft flags
static void finish_qp_shape(DevSkill& S)
{
    S.shape.feedforward = S.shape.multidim = S.shape.conv_last = S.shape.standard = 0;
    S.shape.qp = 1;
    for (int ti = 0; ti < clik::SHAPE_MAX_TASKS; ++ti)
        S.shape.soft[ti] = (ti < S.d.n_tasks && S.d.tasks[ti].soft) ? 1 : 0;
}

// can a shape-specialised QP kernel serve the skill?  (image layout, row budget, LDS)
static bool qp_static_eligible(const DevSkill& S)
{
    if (S.d.n_tasks > clik::SHAPE_MAX_TASKS) return false;
    std::vector<char> img;
    size_t image_bytes = 0;
    if (!build_skill_image(S, img, &image_bytes, sizeof(clik::QpTail))) return false;
    // (the kernels' own count: a joint-limit row and a speed-limit row on the same state are ONE active-set row -
    // a skill with walls, joint limits and speed limits on every joint of a 7-DoF arm has 10 such rows, not 17)
    if (clik::make_qp_plan(S.shape).nr > clik::QPS_MAX_ROWS) return false;
    // (the layout's own slot count: the primal families - bound-constrained, mixed - keep no dual Hessian in LDS, so a
    // two-arm skill with 14 merged box rows fits where the dual form's 14 x 14 + 14 x 14 slots would not)
    const size_t slots = (size_t)clik::qp_slot_layout(S.shape).slots;
    return img.size() + slots * clik::WAVE * sizeof(double) <= clik::kLdsBytesPerCu;
}

static bool build_qp_image(const DevSkill& S, std::vector<char>& out)
{
    size_t image_bytes = 0;
    if (!build_skill_image(S, out, &image_bytes, sizeof(clik::QpTail))) return false;
    clik::QpTail t;
    memset(&t, 0, sizeof(t));
    t.mu = S.qo.weight_shifter;
    for (int j = 0; j < CLIK_MAX_DOF; ++j) t.state_w[j] = S.qo.state_weights[j];
    for (int k = 0; k < CLIK_MAX_QPROWS; ++k) t.slack_w[k] = S.qo.slack_weights[k];
    t.max_iter = S.qo.max_iter;
    memcpy(&out[(image_bytes + 15) & ~(size_t)15], &t, sizeof(t));
    return true;
}

// constraints whose rows are code generated from the caller's expression graph (CLIK_OUT_EXTERN)
// exist only inside the kernel instantiated for them
static bool skill_has_extern(const DevSkill& S)
{
    for (int ti = 0; ti < S.d.n_tasks; ++ti)
        if (S.d.tasks[ti].out_kind[0] == CLIK_OUT_EXTERN || S.d.tasks[ti].attr_ext != 0) return true;
    return false;
}
// ... and so do constraints with more rows than the built-in kernels are wide (CLIK_DYN_MAX_M)
static bool skill_has_wide_task(const DevSkill& S)
{
    for (int ti = 0; ti < S.d.n_tasks; ++ti)
        if (S.d.tasks[ti].m > CLIK_DYN_MAX_M) return true;
    return false;
}
static bool skill_needs_static(const DevSkill& S) { return skill_has_extern(S) || skill_has_wide_task(S); }
static int extern_needs_kernel(const char* what)
{
    return fail(CLIK_EUNSUPPORTED, "%s: the skill has code-generated constraint rows / attributes or a constraint with more "
                                   "than %d rows, and no kernel instantiated for it is attached "
                                   "(casclik_amd.jit needs hipcc)", what, CLIK_DYN_MAX_M);
}

// a handle created without a built-in kernel (more state variables than the dynamic-shape kernels carry) solves only
// through an instantiated kernel: say so with the documented code instead of failing inside the launch
static int no_kernel_for_wide_state(const DevSkill& S, const char* what)
{
    return fail(CLIK_EUNSUPPORTED, "%s: the skill has %d state variables (the built-in kernels carry 8) and no kernel "
                                   "instantiated for it is attached (casclik_amd.jit needs hipcc)", what, S.n);
}

// C++ aggregate initialiser of a ShapeDesc (field order of clik_device.hpp)
static std::string shape_to_string(const clik::ShapeDesc& h)
{
    std::string o = "{";
    auto num = [&](int v) { o += std::to_string(v); o += ", "; };
    auto arr = [&](const int* a, int nn, int used) {
        o += "{";
        for (int i = 0; i < nn; ++i) { o += std::to_string(i < used ? a[i] : 0); if (i + 1 < nn) o += ", "; }
        o += "}, ";
    };
    const int nt = h.n_tasks < clik::SHAPE_MAX_TASKS ? h.n_tasks : clik::SHAPE_MAX_TASKS;
    num(h.n); num(h.n_tasks);
    arr(h.cls, clik::SHAPE_MAX_TASKS, nt); arr(h.m, clik::SHAPE_MAX_TASKS, nt);
    arr(h.flags, clik::SHAPE_MAX_TASKS, nt); arr(h.const_j, clik::SHAPE_MAX_TASKS, nt);
    num(h.all_affine); num(h.uses_fk); num(h.quat_src);
    num(h.feedforward); num(h.multidim); num(h.conv_last); num(h.standard);
    num(h.nj);
    arr(h.jtype, CLIK_MAX_JOINTS, h.nj); arr(h.jq, CLIK_MAX_JOINTS, h.nj); arr(h.jflags, CLIK_MAX_JOINTS, h.nj);
    arr(h.gain_matrix, clik::SHAPE_MAX_TASKS, nt);
    arr(h.ny_terms, clik::SHAPE_MAX_TASKS, nt);
    num(h.n_y);
    arr(h.has_t, clik::SHAPE_MAX_TASKS, nt);
    o += "{";
    for (int i = 0; i < clik::SHAPE_MAX_TASKS; ++i) {
        o += "{";
        for (int k = 0; k < CLIK_MAX_M; ++k) { o += std::to_string(i < nt ? h.ucol[i][k] : 0); if (k + 1 < CLIK_MAX_M) o += ", "; }
        o += (i + 1 < clik::SHAPE_MAX_TASKS) ? "}, " : "}";
    }
    o += "}, ";
    num(h.qp);
    arr(h.soft, clik::SHAPE_MAX_TASKS, nt);
    auto uarr = [&](const unsigned* a, int nn, bool last) {
        o += "{";
        for (int i = 0; i < nn; ++i) { o += std::to_string(a[i]) + "u"; if (i + 1 < nn) o += ", "; }
        o += last ? "}" : "}, ";
    };
    uarr(h.row_nz, clik::SHAPE_MAX_ROWS, false);
    uarr(h.row_one, clik::SHAPE_MAX_ROWS, false);
    o += "{";
    for (int i = 0; i < clik::SHAPE_MAX_TASKS; ++i) {
        o += "{";
        for (int k = 0; k < CLIK_MAX_M; ++k) { o += std::to_string(i < nt ? h.out_nrows[i][k] : 0); if (k + 1 < CLIK_MAX_M) o += ", "; }
        o += (i + 1 < clik::SHAPE_MAX_TASKS) ? "}, " : "}";
    }
    o += "}, " + std::to_string(h.n_x) + ", ";
    o += "{";
    for (int i = 0; i < clik::SHAPE_MAX_TASKS; ++i) { o += std::to_string(i < nt ? h.ext[i] : 0); if (i + 1 < clik::SHAPE_MAX_TASKS) o += ", "; }
    o += "}}";
    return o;
}

// C++ initialiser of the ShapeDesc a skill + options map to (host only, no HIP
// call): the input of tools/gen_shapes.py, which writes clik_shapes_gen.hpp.
extern "C" int clik_shape_describe(const clik_skill_desc* desc, const clik_pinv_opts* opts, char* buf, int cap)
{
    if (!opts || !buf || cap <= 0) return fail(CLIK_EINVAL, "bad arguments");
    std::unique_ptr<DevSkill> S(new (std::nothrow) DevSkill());
    if (!S) return fail(CLIK_ENOMEM, "out of host memory");
    int rc = validate_and_derive(desc, S.get());
    if (rc) return rc;
    finish_pinv_shape(*S, opts);
    const clik::ShapeDesc& h = S->shape;
    const std::string o = shape_to_string(h);
    // (kStaticMaxSets of clik_pinv_kernels.hpp: up to 2^6 mode bodies per kernel)
    bool eligible = S->d.n_tasks <= clik::SHAPE_MAX_TASKS && S->n_sets <= 6;
    {
        std::vector<char> img;
        if (!build_skill_image(*S, img)) eligible = false;      // rows not in task order / too many rows
    }
    // the static plan evaluates the doubly processed first EqualityConstraint in closed form from its own
    // factor or from the host-precomputed inverse of a constant Jacobian (clik_pinv_static.hpp); "standard"
    // keeps the wide-only rule (its tall branch has no damping to carry the closed form)
    for (unsigned act = 0; eligible && act < (1u << S->n_sets); ++act) {
        int r = 0, set_idx = 0;
        for (int ti = 0; ti < h.n_tasks; ++ti) {
            const int cls = h.cls[ti];
            if (cls == CLIK_CLS_VELSET) continue;
            if (cls == CLIK_CLS_SET) {
                const bool active = (act >> set_idx) & 1u;
                ++set_idx;
                if (!active) continue;
            }
            const bool conv = cls == CLIK_CLS_SET && ti == h.n_tasks - 1 && h.conv_last;
            const bool contributes = cls == CLIK_CLS_EQ || cls == CLIK_CLS_VELEQ || conv;
            if (contributes && r == 0 && cls == CLIK_CLS_EQ) {
                const bool wide = h.standard ? (h.m[ti] < h.n) : (h.n >= h.m[ti]);
                if (!wide && h.standard) eligible = false;
            }
            r += h.m[ti];
        }
    }
    if ((int)o.size() + 1 > cap) return fail(CLIK_EINVAL, "buffer too small");
    memcpy(buf, o.c_str(), o.size() + 1);
    return eligible ? 1 : 0;
}

// CLIK_HOST_ONLY=1: handles are created WITHOUT touching a device (no allocation, no upload) - for the host-side
// queries only (clik_*_image_words, kernel names): casclik_amd/jit.py uses it to instantiate value-specialised kernels
// ahead of time on a machine without a GPU.  Every solve / rollout / data entry point refuses such a handle.
// (clik_*_create_host ask for it explicitly, per call and per thread; the environment variable remains for whole processes)
static thread_local bool g_host_only_call = false;
static bool host_only_mode()
{
    if (g_host_only_call) return true;
    const char* e = getenv("CLIK_HOST_ONLY");
    return e && e[0] == '1';
}
#define CLIK_NEEDS_DEVICE_HANDLE(h)                                                                        \
    do {                                                                                                   \
        if ((h) && (h)->dev == nullptr)                                                                    \
            return fail(CLIK_EINVAL, "this handle was created host-only (clik_*_create_host / CLIK_HOST_ONLY=1): host-side queries only"); \
    } while (0)

// one copy of the skill image on the device, owned by the handle (h->d_img, null on failure)
static hipError_t upload_image(clik_handle* h, const std::vector<char>& img)
{
    hipError_t e = hipMalloc(&h->d_img, img.size());
    if (e == hipSuccess) e = hipMemcpy(h->d_img, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess && h->d_img) {
        (void)hipFree(h->d_img);
        h->d_img = nullptr;
    }
    return e;
}

// the DevSkill record on the device (h->dev), unless the handle is host-only
static int upload_skill(clik_handle* h)
{
    if (host_only_mode()) return CLIK_OK;
    hipError_t e = hipMalloc((void**)&h->dev, sizeof(DevSkill));
    if (e != hipSuccess) return hipfail(e, "hipMalloc(skill)");
    e = hipMemcpy(h->dev, &h->host, sizeof(DevSkill), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hipfail(e, "hipMemcpy(skill)");
    return CLIK_OK;
}

extern "C" int clik_pinv_create(const clik_skill_desc* desc, const clik_pinv_opts* opts, clik_pinv** out)
{
    if (!out) return fail(CLIK_EINVAL, "null out pointer");
    *out = nullptr;
    if (!opts) return fail(CLIK_EINVAL, "null options");
    std::unique_ptr<clik_pinv> h(new (std::nothrow) clik_pinv());
    if (!h) return fail(CLIK_ENOMEM, "out of host memory");
    int used_rows = 0;
    int rc = validate_and_derive(desc, &h->host, &used_rows);
    if (rc) return rc;
    DevSkill& S = h->host;
    finish_pinv_shape(S, opts);
    if (opts->pinv_method != CLIK_PINV_DAMPED && opts->pinv_method != CLIK_PINV_STANDARD)
        return fail(CLIK_EINVAL, "pinv_method must be damped or standard");
    if (S.n_sets > CLIK_MAX_SETS)
        return fail(CLIK_EUNSUPPORTED, "%d SetConstraints give 2^%d modes (limit %d sets)", S.n_sets, S.n_sets,
                    CLIK_MAX_SETS);
    for (int ti = 0; ti < S.d.n_tasks; ++ti) {
        const clik_task& t = S.d.tasks[ti];
        if (t.cls == CLIK_CLS_SET && t.m > 1 && !opts->multidim_sets)
            // same refusal as pseudo_inverse.py:299-312
            return fail(CLIK_EUNSUPPORTED,
                        "PseudoInverseController does not yet have guaranteed stable support for "
                        "multidimensional SetConstraints (task %d has %d rows). Set the multidim_sets "
                        "field in options to True for experimental support.", ti, t.m);
    }
    // mode table (pseudo_inverse.py:107-130): bit k <-> k-th SetConstraint in
    // priority order; patterns stably sorted by the number of active sets
    S.n_modes = 1 << S.n_sets;
    {
        int k = 0;
        for (int pc = 0; pc <= S.n_sets; ++pc)
            for (int v = 0; v < S.n_modes; ++v)
                if (popcount32((unsigned)v) == pc) S.act[k++] = (uint32_t)v;
    }
    S.last_set_converges = (S.d.n_tasks > 0 && S.d.tasks[S.d.n_tasks - 1].cls == CLIK_CLS_SET &&
                            opts->converge_final_set_to_max) ? 1 : 0;
    for (int ti = 0; ti < S.d.n_tasks; ++ti) {
        if (!S.task_const_j[ti]) continue;
        const clik_task& t = S.d.tasks[ti];
        double J[CLIK_MAX_M * CLIK_MAX_DOF];
        for (int i = 0; i < t.m; ++i)
            for (int j = 0; j < S.n; ++j) J[i * S.n + j] = S.d.rows[t.out_row0[i]].a[j];
        if (!host_const_pinv(*opts, t.m, S.n, J, S.cpinv[ti])) {
            // singular Gram matrix (pinv_method "standard" on a rank-deficient
            // task): let the device run the generic solve like the reference would
            S.task_const_j[ti] = 0;
            if (ti < clik::SHAPE_MAX_TASKS) S.shape.const_j[ti] = 0;
        }
    }
    {
        // CLIK_FORCE_DYNAMIC=1: dynamic kernel only; CLIK_NO_AOT=1: skip the AOT table
        // (the Python layer may still attach a run-time instantiated kernel)
        const char* force = getenv("CLIK_FORCE_DYNAMIC");
        const char* noaot = getenv("CLIK_NO_AOT");
        h->kernel = clik::pinv_pick_kernel(S, ((force && force[0] == '1') || (noaot && noaot[0] == '1')) ? 0 : 1);
    }
    if (h->kernel < 0 && !skill_has_wide_task(S) && S.n <= 8)
        return fail(CLIK_EUNSUPPORTED, "no kernel variant for n = %d", S.n);
    // (kernel < 0 with a wide constraint or with more than eight state variables - a 7-DoF arm with two or three
    // virtual variables, CLIK_MAX_DOF = 10: no built-in kernel is wide enough; the handle solves once a kernel
    // instantiated for the skill is attached, and answers CLIK_EUNSUPPORTED until then)
    compute_warm(S, used_rows, h->warm);
    S.lds_slots = clik::pinv_lds_slots_host(clik::pinv_kernel_width(h->kernel), S.d.n_y);
    if ((size_t)S.lds_slots * clik::WAVE * sizeof(double) > clik::kLdsBytesPerCu)
        return fail(CLIK_EUNSUPPORTED, "skill needs %d LDS slots per lane (input_var too large)", S.lds_slots);
    rc = upload_skill(h.get());
    if (rc) return rc;
    if (h->dev && clik::pinv_kernel_is_static(h->kernel)) {
        std::vector<char> img;
        if (!build_skill_image(S, img)) {
            // rows not laid out contiguously: serve the skill with the dynamic kernel
            h->kernel = clik::pinv_pick_kernel(S, 0);
        } else {
            const hipError_t e = upload_image(h.get(), img);
            if (e != hipSuccess) return hipfail(e, "skill image upload");
        }
    }
    {
        // The measuring switches of the kernel choice (pinv_select, clik_pinv_select.hpp), each off with a leading '0'.
        // CLIK_MODE_PARALLEL: small batches (fewer wavefronts than SIMDs) evaluate the modes of a skill with one or two
        // SetConstraints speculatively, one wave per mode on the same 64 instances (pinv_solve_static_mp_kernel;
        // measured 8.0 -> 7.2 us on the config-3 stack, "mixed").
        // CLIK_LANES: unset / empty / 0 = the library's choice, 4 = the team kernel (four lanes per instance) of the
        // config-3 family at every batch size (head-to-head runs), anything else = the lane-per-instance kernels.
        // CLIK_LARGE_BATCH: the two-waves-per-SIMD lane kernel from kOcc2MinBatch instances on, which only the
        // ahead-of-time table carries.  CLIK_QUAD_FRONT: four lanes per instance for small batches of single-mode skills.
        const char* mp = getenv("CLIK_MODE_PARALLEL");
        const char* ln = getenv("CLIK_LANES");
        const char* lb = getenv("CLIK_LARGE_BATCH");
        const char* qf = getenv("CLIK_QUAD_FRONT");
        h->policy.mode_waves = !(mp && mp[0] == '0');
        h->policy.lanes = (!ln || ln[0] == '0' || ln[0] == '\0') ? clik::PinvLanes::choice
                          : ln[0] == '4'                         ? clik::PinvLanes::team
                                                                 : clik::PinvLanes::lane;
        h->policy.large_batch = !(lb && lb[0] == '0');
        h->policy.aot_large_batch_build = clik::pinv_kernel_is_static(h->kernel) != 0;
        h->policy.quad_front = !(qf && qf[0] == '0');
    }
    *out = h.release();
    return CLIK_OK;
}

// Attach a shape-specialised kernel instantiated at run time for this handle's
// skill (casclik_amd/jit.py compiles clik_pinv_kernels.hpp for the ShapeDesc that
// clik_shape_describe printed).  Mirrors the reference's JIT at
// setup_problem_functions (pseudo_inverse.py:476-483).
extern "C" int clik_pinv_attach_kernel(clik_pinv* h, void* solve_fn, void* rollout_fn, const char* name)
{
    // (rollout_fn may be NULL: the rollout then keeps the kernel chosen at creation)
    if (!h || !solve_fn) return fail(CLIK_EINVAL, "null argument");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (!h->d_img) {
        std::vector<char> img;
        if (!build_skill_image(h->host, img))
            return fail(CLIK_EUNSUPPORTED, "skill rows are not contiguous: no static kernel possible");
        const hipError_t e = upload_image(h, img);
        if (e != hipSuccess) return hipfail(e, "skill image upload");
    }
    h->jit_solve = (clik_jit_solve_fn)solve_fn;
    h->jit_rollout = (clik_jit_rollout_fn)rollout_fn;
    snprintf(h->jit_name, sizeof(h->jit_name), "%s", name ? name : "jit");
    return CLIK_OK;
}

extern "C" int clik_pinv_attach_value_kernel(clik_pinv* h, void* solve_fn, void* rollout_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (solve_fn && !clik::shape_team_ok(h->host.shape) && !clik::shape_value_lane_ok(h->host.shape))
        return fail(CLIK_EUNSUPPORTED, "value-specialised kernels exist for the four-lanes-per-instance family and for "
                                       "single-mode skills without virtual variables");
    h->val_solve = (clik_jit_value_fn)solve_fn;
    h->val_rollout = solve_fn ? (clik_jit_rollout_fn)rollout_fn : nullptr;
    h->policy.values_attached = solve_fn != nullptr;
    return CLIK_OK;
}

static int fill_tick(const DevSkill& S, const double* tterms, TickArgs* tk)
{
    memset(tk, 0, sizeof(*tk));
    const int nts = S.d.n_tslots;
    if (nts > 0) {
        if (!tterms) return fail(CLIK_EINVAL, "skill has %d time slots but tterms is NULL", nts);
        memcpy(tk->tv, tterms, sizeof(double) * 2 * nts);
    }
    return CLIK_OK;
}

// ---- what the launch paths check the same way ----------------------------------------------------------------------------
static int input_var_check(const DevSkill& S, const double* y)
{
    if (S.d.n_y > 0 && !y) return fail(CLIK_EINVAL, "skill has input_var: y required");
    return CLIK_OK;
}

// x / dx of a skill with virtual variables (`x_hint`: what a rollout's refusal adds - the entry point that takes x)
static int virtual_var_check(const DevSkill& S, const double* x, const double* dx, const char* x_hint = "")
{
    if (S.d.n_x > 0 && (!x || !dx)) return fail(CLIK_EINVAL, "skill has virtual_var: x and dx required%s", x_hint);
    return CLIK_OK;
}

// q / dq, then y of a skill with input_var
static int joint_args_check(const DevSkill& S, const double* q, const double* y, const double* dq)
{
    if (!q || !dq) return fail(CLIK_EINVAL, "q and dq must be device pointers");
    return input_var_check(S, y);
}

// the state a tick or rollout reads and the rates it writes (device), checked in this order everywhere.  (The rollouts that
// ask for x / dx BEFORE their kernel-presence checks call the two halves themselves, each at its place.)
static int state_args_check(const DevSkill& S, const double* q, const double* x, const double* y, const double* dq,
                            const double* dx)
{
    const int rc = virtual_var_check(S, x, dx);
    return rc ? rc : joint_args_check(S, q, y, dq);
}

// controller evaluations per tick of an integration scheme (`who`: the prefix of the QP rollouts' refusal)
static int stages_of(int32_t method, int* stages, const char* who = "")
{
    if (method != CLIK_INTEGRATE_EULER && method != CLIK_INTEGRATE_RK4)
        return fail(CLIK_EINVAL, "%sunknown integration method %d", who, method);
    *stages = method == CLIK_INTEGRATE_RK4 ? 4 : 1;
    return CLIK_OK;
}

// what the pseudo-inverse launchers take next to the batch: the handle's skill and policy, the virtual variables of a
// rollout, its stages, the per-instance times of a tick, the records of a recording rollout
static clik::LaunchArgs launch_args(const clik_pinv* h, double* x, double* dx, int stages, const double* t_inst,
                                    const clik::RollRec* rec)
{
    const DevSkill& S = h->host;
    return {h->dev, h->d_img, &h->warm, S.d.n_q, S.d.n_x, S.d.n_y, h->policy, x, dx, stages, t_inst, rec};
}

extern "C" int clik_pinv_attach_resident_kernel(clik_pinv* h, void* resident_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (resident_fn && !clik::shape_team_ok(h->host.shape) && !clik::shape_quad_front_ok(h->host.shape))
        return fail(CLIK_EUNSUPPORTED, "resident ticks exist for the four-lanes-per-instance kernels only (the config-3 family, "
                                       "single-mode skills with forward kinematics)");
    h->val_resident = (decltype(h->val_resident))resident_fn;
    return CLIK_OK;
}

extern "C" int clik_pinv_resident_waves(const clik_pinv* h, int64_t B)
{
    if (!h || B <= 0) return fail(CLIK_EINVAL, "bad arguments");
    // (the config-3 family runs four waves per 64 instances, the single-mode skills one wave per 16: one slot per wave)
    if (!clik::shape_team_ok(h->host.shape) && clik::shape_quad_front_ok(h->host.shape)) return (int)((B + 15) / 16);
    return clik::team_waves_rt((long long)B);
}

static int resident_run_common(const clik_pinv* h, int64_t B, int32_t n_ticks, const double* tterms, const double* q,
                               const double* y, double* dq, int32_t* mode, clik_ticket* ticket, uint32_t* done,
                               double integrate_dt, double max_speed, double timeout_s, void* stream);

extern "C" int clik_pinv_resident_run(const clik_pinv* h, int64_t B, int32_t n_ticks, const double* tterms,
                                      const double* q, const double* y, double* dq, int32_t* mode,
                                      clik_ticket* ticket, uint32_t* done, double timeout_s, void* stream)
{
    return resident_run_common(h, B, n_ticks, tterms, q, y, dq, mode, ticket, done, 0.0, 0.0, timeout_s, stream);
}

extern "C" int clik_pinv_resident_run_state(const clik_pinv* h, int64_t B, int32_t n_ticks, const double* tterms,
                                            const double* q, const double* y, double* dq, int32_t* mode,
                                            clik_ticket* ticket, uint32_t* done, double integrate_dt, double max_speed,
                                            double timeout_s, void* stream)
{
    if (!(integrate_dt > 0.0)) return fail(CLIK_EINVAL, "integrate_dt must be positive");
    if (max_speed < 0.0) return fail(CLIK_EINVAL, "max_speed must not be negative (0: no clamp)");
    return resident_run_common(h, B, n_ticks, tterms, q, y, dq, mode, ticket, done, integrate_dt, max_speed, timeout_s,
                               stream);
}

// what the resident runs of both controllers check before they launch (`attached`: the handle has its resident kernel;
// `missing`: what to say when not) and the one record of time terms they run with
static int resident_checks(const clik_handle* h, bool attached, const char* missing, int64_t B, int32_t n_ticks,
                           const double* tterms, const double* q, const double* y, const double* dq,
                           const clik_ticket* ticket, const uint32_t* done, double timeout_s, TickArgs* tk)
{
    if (!attached) return fail(CLIK_EUNSUPPORTED, "%s", missing);
    if (B <= 0 || n_ticks <= 0) return fail(CLIK_EINVAL, "B and n_ticks must be positive");
    if (!q || !dq || !ticket || !done) return fail(CLIK_EINVAL, "q, dq, ticket and done must be device pointers");
    const int rc = input_var_check(h->host, y);
    if (rc) return rc;
    if (!(timeout_s > 0.0) || timeout_s > 60.0) return fail(CLIK_EINVAL, "timeout_s must lie in (0, 60]");
    return fill_tick(h->host, tterms, tk);
}

static int resident_run_common(const clik_pinv* h, int64_t B, int32_t n_ticks, const double* tterms, const double* q,
                               const double* y, double* dq, int32_t* mode, clik_ticket* ticket, uint32_t* done,
                               double integrate_dt, double max_speed, double timeout_s, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    TickArgs tk;
    const int rc = resident_checks(h, h->val_resident != nullptr,
                                   "resident ticks need the value-specialised kernel of the four-lanes-per-instance "
                                   "family attached to this handle (none is)",
                                   B, n_ticks, tterms, q, y, dq, ticket, done, timeout_s, &tk);
    if (rc) return rc;
    // (every wave of the launch must be resident at once: the launch wrapper of the instantiated kernel checks the grid
    // against that kernel's occupancy on this device and answers hipErrorNotSupported beyond it)
    // (watchdog budget: polls at a nominal 0.2 us each - a load that hits the L2 plus s_sleep 1; round 6 found the
    // budget of the earlier 2.5 us figure used up in a tenth of timeout_s)
    unsigned long long budget = (unsigned long long)(timeout_s * 5e6);
    if (integrate_dt > 0.0) {
        // the step and the clamp travel in the ticket (stream-ordered in front of the kernel); bit 63 of the budget
        // picks the instantiation that keeps the state
        const double pair[2] = {integrate_dt, max_speed};
        hipError_t ce = hipMemcpyAsync(&ticket->integrate_dt, pair, sizeof(pair), hipMemcpyHostToDevice, (hipStream_t)stream);
        if (ce != hipSuccess) return hipfail(ce, "resident ticks: writing the integration step into the ticket");
        budget |= 1ull << 63;
    }
    hipError_t e = h->val_resident(&tk, (long long)B, q, y, dq, mode, (void*)ticket, (unsigned*)done, n_ticks, budget,
                                   (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(CLIK_EUNSUPPORTED, "resident ticks: %lld instances need more blocks than this kernel can keep resident "
                                       "at once on this device (every wave must be running for a tick to complete)",
                    (long long)B);
    if (e != hipSuccess) return hipfail(e, "resident kernel launch");
    return CLIK_OK;
}

extern "C" int clik_ticket_feed(clik_ticket* ticket, const uint32_t* done, int32_t n_ticks, int32_t closed_loop,
                                int32_t waves_per_tick, double timeout_s, void* stream)
{
    if (!ticket || !done || n_ticks <= 0 || waves_per_tick <= 0) return fail(CLIK_EINVAL, "bad arguments");
    if (!(timeout_s > 0.0) || timeout_s > 60.0) return fail(CLIK_EINVAL, "timeout_s must lie in (0, 60]");
    hipError_t e = clik::launch_ticket_feed((void*)ticket, (const unsigned*)done, n_ticks, closed_loop, (unsigned)waves_per_tick,
                                            (unsigned long long)(timeout_s * 5e6), (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "ticket feeder launch");
    return CLIK_OK;
}

// the skill image of this handle (what the static kernels read from memory) as 64-bit words, for
// casclik_amd/jit.py to compile into a value-specialised kernel; returns the number of words
extern "C" int clik_pinv_image_words(const clik_pinv* h, uint64_t* buf, int cap)
{
    if (!h || !buf || cap <= 0) return fail(CLIK_EINVAL, "bad arguments");
    std::vector<char> img;
    size_t bytes = 0;
    if (!build_skill_image(h->host, img, &bytes)) return fail(CLIK_EUNSUPPORTED, "skill rows are not contiguous");
    const int words = (int)((bytes + 7) / 8);
    if (words > cap) return fail(CLIK_EINVAL, "image needs %d words, buffer holds %d", words, cap);
    memcpy(buf, img.data(), (size_t)words * 8);
    return words;
}

extern "C" int clik_pinv_create_host(const clik_skill_desc* desc, const clik_pinv_opts* opts, clik_pinv** out)
{
    g_host_only_call = true;
    const int rc = clik_pinv_create(desc, opts, out);
    g_host_only_call = false;
    return rc;
}
extern "C" int clik_qp_create_host(const clik_skill_desc* desc, const clik_qp_opts* opts, clik_qp** out)
{
    g_host_only_call = true;
    const int rc = clik_qp_create(desc, opts, out);
    g_host_only_call = false;
    return rc;
}

extern "C" int clik_pinv_destroy(clik_pinv* h)
{
    delete h;       // (the handle releases what it holds on the device)
    return CLIK_OK;
}

extern "C" int clik_pinv_n_modes(const clik_pinv* h) { return h ? h->host.n_modes : 0; }
extern "C" const char* clik_pinv_kernel_name(const clik_pinv* h)
{
    if (h && h->jit_solve) return h->jit_name;
    return h ? clik::pinv_kernel_name(h->kernel) : "none";
}

extern "C" const char* clik_pinv_kernel_variant(const clik_pinv* h, int64_t B)
{
    if (!h) return "none";
    if (!h->jit_solve && !(h->kernel >= 0 && clik::pinv_kernel_is_static(h->kernel))) return "dynamic";
    return clik::kPinvVariantName[(int)clik::pinv_select(h->host.shape, h->policy, (long long)B, clik::PinvOp::tick)];
}

static int pinv_solve_common(const clik_pinv* h, int64_t B, const double* tterms, const double* t_inst,
                             const double* q, const double* x, const double* y, double* dq, double* dx,
                             int32_t* mode, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (B < 0) return fail(CLIK_EINVAL, "negative batch size");
    if (B == 0) return CLIK_OK;
    const DevSkill& S = h->host;
    int rc = state_args_check(S, q, x, y, dq, dx);
    if (rc) return rc;
    const bool is_static = h->jit_solve || (h->kernel >= 0 && clik::pinv_kernel_is_static(h->kernel));
    if (!is_static && skill_needs_static(S)) return extern_needs_kernel("clik_pinv_solve_batch");
    if (h->kernel < 0 && !h->jit_solve) return no_kernel_for_wide_state(S, "clik_pinv_solve_batch");
    TickArgs tk;
    if (t_inst == nullptr) {
        rc = fill_tick(S, tterms, &tk);
        if (rc) return rc;
    } else if (!is_static) {
        return fail(CLIK_EUNSUPPORTED, "clik_pinv_solve_batch_t: per-instance time needs a shape-specialised kernel "
                                       "for the skill (none built in, none attached)");
    }
    const clik::LaunchArgs la = launch_args(h, nullptr, nullptr, 1, t_inst, nullptr);
    // (the value-specialised library evaluates its own batch limits - it may have been built with other
    // CLIK_VALUE_LANE_* settings than this one: hipErrorNotSupported means "not mine", and the image-reading
    // kernels take the call)
    hipError_t e = hipErrorNotSupported;
    if (h->val_solve && t_inst == nullptr &&
        clik::pinv_value_variant(clik::pinv_select(S.shape, h->policy, (long long)B, clik::PinvOp::tick)))
        e = h->val_solve(&la, &tk, (long long)B, q, y, dq, mode, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        e = h->jit_solve
                ? h->jit_solve(&la, &tk, (long long)B, q, x, y, dq, dx, mode, (hipStream_t)stream)
                : clik::pinv_launch_solve(h->kernel, la, tk, (long long)B, q, x, y, dq, dx, mode,
                                          (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "pinv_solve_kernel launch");
    return CLIK_OK;
}

extern "C" int clik_pinv_solve_batch(const clik_pinv* h, int64_t B, const double* tterms, const double* q,
                                     const double* x, const double* y, double* dq, double* dx,
                                     int32_t* mode, void* stream)
{
    return pinv_solve_common(h, B, tterms, nullptr, q, x, y, dq, dx, mode, stream);
}

extern "C" int clik_pinv_solve_batch_t(const clik_pinv* h, int64_t B, const double* t_inst, const double* q,
                                       const double* x, const double* y, double* dq, double* dx,
                                       int32_t* mode, void* stream)
{
    if (h && h->host.d.n_tslots > 0 && !t_inst)
        return fail(CLIK_EINVAL, "clik_pinv_solve_batch_t: t_inst (device, [B][2 * n_tslots]) required");
    if (h && h->host.d.n_tslots == 0)       // (nothing depends on time)
        return pinv_solve_common(h, B, nullptr, nullptr, q, x, y, dq, dx, mode, stream);
    return pinv_solve_common(h, B, nullptr, t_inst, q, x, y, dq, dx, mode, stream);
}

// Time-slot records of a rollout (host) -> a device buffer that lives for this call only: allocated, filled and
// released in stream order (hipMallocAsync / hipFreeAsync), so handles stay immutable and two rollouts on two
// streams never share it.  The host array is consumed before the call returns BY CONSTRUCTION: it is copied into a
// pinned staging slot of a process-wide pool here (a plain memcpy), and the asynchronous host-to-device copy reads
// that slot, so nothing depends on how the runtime treats a pageable source and the call never waits for the
// stream.  A slot is reused once the event recorded behind its copy has completed.  (A rollout with time slots is
// therefore not graph-capturable - its records are consumed at call time; a skill without time slots stages
// nothing and captures like a tick.  The clik_*_rollout_batch_dev calls consume nothing on the host at call time and use
// no pinned slot: their tick times are a device array and the time kernel fills the records on the stream, see
// rollout_tterms.)
namespace {
// The record buffer of one rollout call (null: the skill has no time slots).  Whoever holds it releases it in stream
// order - hipFreeAsync on the stream it was made on - when it goes out of scope: a launch path keeps it until it
// returns, so the release is enqueued behind the launch.
struct TtBuffer {
    double* ptr = nullptr;
    hipStream_t stream = nullptr;
    TtBuffer() = default;
    TtBuffer(TtBuffer&& o) noexcept : ptr(o.ptr), stream(o.stream) { o.ptr = nullptr; }
    TtBuffer(const TtBuffer&) = delete;
    TtBuffer& operator=(const TtBuffer&) = delete;
    TtBuffer& operator=(TtBuffer&&) = delete;
    ~TtBuffer()
    {
        if (ptr) (void)hipFreeAsync(ptr, stream);
    }
};
struct StageSlot { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool busy = false; int dev = -1; };
std::mutex g_stage_mu;
std::vector<StageSlot> g_stage_slots;
}

static int stage_tterms(const double* tterms, size_t count, hipStream_t stream, TtBuffer* out)
{
    if (count == 0) return CLIK_OK;
    if (!tterms) return fail(CLIK_EINVAL, "tterms required");
    const size_t bytes = count * sizeof(double);
    int dev = 0;
    (void)hipGetDevice(&dev);
    StageSlot* slot = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (auto& sl : g_stage_slots) {
            if (sl.dev != dev || sl.cap < bytes) continue;
            if (sl.busy && hipEventQuery(sl.done) != hipSuccess) continue;
            slot = &sl;
            break;
        }
        if (!slot) {
            StageSlot sl;
            sl.cap = bytes < 4096 ? 4096 : bytes;
            sl.dev = dev;
            hipError_t e = hipHostMalloc(&sl.host, sl.cap, hipHostMallocDefault);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
            if (e != hipSuccess) {
                if (sl.host) (void)hipHostFree(sl.host);
                return hipfail(e, "pinned staging slot (tterms)");
            }
            g_stage_slots.reserve(64);          // (pointers into the vector are taken under the lock only)
            g_stage_slots.push_back(sl);
            slot = &g_stage_slots.back();
        }
        slot->busy = true;
        std::memcpy(slot->host, tterms, bytes);
        out->stream = stream;
        hipError_t e = hipMallocAsync((void**)&out->ptr, bytes, stream);
        if (e != hipSuccess) {
            out->ptr = nullptr;
            slot->busy = false;
            return hipfail(e, "hipMallocAsync(tterms)");
        }
        e = hipMemcpyAsync(out->ptr, slot->host, bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(slot->done, stream);
        if (e != hipSuccess) return hipfail(e, "hipMemcpyAsync(tterms)");       // (the caller leaves, and `out` releases it)
    }
    return CLIK_OK;
}

// Where the time-slot records of a rollout come from: a host table (`host`, staged as above) or - `on_device` - the tick
// times as a device array, from which the handle's time kernel fills the records in stream order.
struct TtSource {
    const double* host;
    const double* times;
    clik_time_fn time_fn;
    bool on_device;
};
static TtSource tt_host(const double* tterms) { return TtSource{tterms, nullptr, nullptr, false}; }
static TtSource tt_device(const double* times, clik_time_fn fn) { return TtSource{nullptr, times, fn, true}; }

// the stream-ordered record buffer of one rollout call, filled from `src` into `out` (an empty one, the caller's)
static int rollout_tterms(const TtSource& src, int n_tslots, int n_ticks, int stages, double dt, hipStream_t stream,
                          TtBuffer* out)
{
    const size_t count = (size_t)n_ticks * stages * 2 * (size_t)n_tslots;
    if (!src.on_device) return stage_tterms(src.host, count, stream, out);
    if (count == 0) return CLIK_OK;
    if (!src.times) return fail(CLIK_EINVAL, "times (device, [n_ticks]) required: the skill has time slots");
    if (!src.time_fn)
        return fail(CLIK_EUNSUPPORTED, "no time kernel attached for this skill (clik_*_attach_time_kernel)");
    out->stream = stream;
    hipError_t e = hipMallocAsync((void**)&out->ptr, count * sizeof(double), stream);
    if (e != hipSuccess) {
        out->ptr = nullptr;
        return hipfail(e, "hipMallocAsync(tterms)");
    }
    e = src.time_fn(src.times, (long long)n_ticks, stages, dt, out->ptr, stream);
    if (e != hipSuccess) return hipfail(e, "time kernel launch");       // (the caller leaves, and `out` releases it)
    return CLIK_OK;
}

// ---- entry points that do not depend on the controller: written once over the base, forwarded to per controller -------
static int attach_time_kernel(clik_handle* h, void* time_terms_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    h->time_fn = (clik_time_fn)time_terms_fn;
    return CLIK_OK;
}

static int time_terms(const clik_handle* h, int64_t n_times, const double* times, int32_t stages, double dt, double* out,
                      void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (n_times < 0) return fail(CLIK_EINVAL, "negative size");
    if (stages != 1 && stages != 4) return fail(CLIK_EINVAL, "stages must be 1 or 4, got %d", stages);
    if (h->host.d.n_tslots == 0 || n_times == 0) return CLIK_OK;
    if (!h->time_fn) return fail(CLIK_EUNSUPPORTED, "no time kernel attached for this skill (clik_*_attach_time_kernel)");
    if (!times || !out) return fail(CLIK_EINVAL, "times and out must be device pointers");
    const hipError_t e = h->time_fn(times, (long long)n_times, stages, dt, out, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "time kernel launch");
    return CLIK_OK;
}

extern "C" int clik_pinv_attach_time_kernel(clik_pinv* h, void* fn) { return attach_time_kernel(h, fn); }
extern "C" int clik_qp_attach_time_kernel(clik_qp* h, void* fn) { return attach_time_kernel(h, fn); }
extern "C" int clik_pinv_time_terms(const clik_pinv* h, int64_t n_times, const double* times, int32_t stages, double dt,
                                    double* out, void* stream)
{
    return time_terms(h, n_times, times, stages, dt, out, stream);
}
extern "C" int clik_qp_time_terms(const clik_qp* h, int64_t n_times, const double* times, int32_t stages, double dt,
                                  double* out, void* stream)
{
    return time_terms(h, n_times, times, stages, dt, out, stream);
}

extern "C" int clik_pinv_rollout_batch(const clik_pinv* hc, int64_t B, int32_t n_ticks, double dt,
                                       double max_speed, const double* tterms, double* q, const double* y,
                                       double* dq, int32_t* mode, void* stream)
{
    return clik_pinv_rollout_batch_x(hc, B, n_ticks, dt, max_speed, tterms, q, nullptr, y, dq, nullptr, mode, stream);
}

extern "C" int clik_pinv_rollout_batch_x(const clik_pinv* hc, int64_t B, int32_t n_ticks, double dt,
                                         double max_speed, const double* tterms, double* q, double* x,
                                         const double* y, double* dq, double* dx, int32_t* mode, void* stream)
{
    return clik_pinv_rollout_batch_m(hc, B, n_ticks, CLIK_INTEGRATE_EULER, dt, max_speed, tterms, q, x, y, dq, dx, mode,
                                     stream);
}

// what _rec adds to _m, checked: the RollRec the kernels take, or an error
static int roll_rec_of(int64_t B, int n_y, int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                       double* rec_x, double* rec_dx, double* rec_slack, int32_t* rec_flag, clik::RollRec* rr)
{
    if (record_every < 0) return fail(CLIK_EINVAL, "record_every must be 0 (no records) or the number of ticks per record");
    rr->y_stride = (y_per_tick != 0 && n_y > 0) ? (long long)B * n_y : 0;
    rr->every = record_every;
    rr->q = rec_q;
    rr->dq = rec_dq;
    rr->x = rec_x;
    rr->dx = rec_dx;
    rr->slack = rec_slack;
    rr->flag = rec_flag;
    return CLIK_OK;
}

static int pinv_rollout_common(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                               double max_speed, const TtSource& tts, double* q, double* x, const double* y,
                               double* dq, double* dx, int32_t* mode, void* stream, const clik::RollRec* rec);

// do shape-specialised kernels serve the rollouts of this handle: an attached one or one of the table's?  (The ticks ask
// for jit_solve instead, see pinv_solve_common: a skill with many SetConstraints has that and no jit_rollout.)
static bool pinv_shape_served(const clik_pinv* h)
{
    return h->jit_rollout || (h->kernel >= 0 && clik::pinv_kernel_is_static(h->kernel));
}

extern "C" int clik_pinv_rollout_batch_m(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                         double max_speed, const double* tterms, double* q, double* x,
                                         const double* y, double* dq, double* dx, int32_t* mode, void* stream)
{
    return pinv_rollout_common(h, B, n_ticks, method, dt, max_speed, tt_host(tterms), q, x, y, dq, dx, mode, stream, nullptr);
}

extern "C" int clik_pinv_rollout_batch_rec(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                           double max_speed, const double* tterms, double* q, double* x,
                                           const double* y, double* dq, double* dx, int32_t* mode, void* stream,
                                           int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                           double* rec_x, double* rec_dx, int32_t* rec_mode)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    clik::RollRec rr;
    int rc = roll_rec_of(B, h->host.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, nullptr, rec_mode, &rr);
    if (rc) return rc;
    return pinv_rollout_common(h, B, n_ticks, method, dt, max_speed, tt_host(tterms), q, x, y, dq, dx, mode, stream, &rr);
}

extern "C" int clik_pinv_rollout_batch_dev(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                           double max_speed, const double* times, double* q, double* x,
                                           const double* y, double* dq, double* dx, int32_t* mode, void* stream,
                                           int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                           double* rec_x, double* rec_dx, int32_t* rec_mode)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    const TtSource tts = tt_device(times, h->time_fn);
    // (no records and no per-tick targets: the plain rollout kernels, as clik_pinv_rollout_batch_m)
    if (record_every == 0 && y_per_tick == 0)
        return pinv_rollout_common(h, B, n_ticks, method, dt, max_speed, tts, q, x, y, dq, dx, mode, stream, nullptr);
    clik::RollRec rr;
    int rc = roll_rec_of(B, h->host.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, nullptr, rec_mode, &rr);
    if (rc) return rc;
    return pinv_rollout_common(h, B, n_ticks, method, dt, max_speed, tts, q, x, y, dq, dx, mode, stream, &rr);
}

// ---- attaching the on-demand kernels (recording, constraint values, summaries, summarising and converging rollouts) ---
// The family check of a controller: does a shape-specialised kernel serve this handle (`refusal` says what exists only
// then), and is its image on the device?
static int pinv_attach_checks(clik_pinv* h, const char* refusal)
{
    if (!h->jit_solve && !pinv_shape_served(h)) return fail(CLIK_EUNSUPPORTED, "%s", refusal);
    if (!h->d_img) return fail(CLIK_EUNSUPPORTED, "no skill image on the device: attach the kernel first");
    return CLIK_OK;
}
// ... of the QP controller: the skill is in the shape-specialised family; its image is uploaded here when no kernel of
// that family runs yet (one refusal text for every kernel: kQpFamily)
static int qp_attach_checks(clik_qp* h, const char* refusal);
static const char* const kQpFamily = "skill is outside the shape-specialised QP family";

// What every clik_*_attach_*_kernel of an on-demand kernel does: store `fn` in `slot` - attaching (fn non-null) needs a
// device handle that passes the controller's family check, detaching needs nothing.
template <class H, class Base, class Fn>
static int attach_on_demand(H* h, Fn Base::*slot, void* fn, int (*family)(H*, const char*), const char* refusal)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (fn) {
        CLIK_NEEDS_DEVICE_HANDLE(h);
        const int rc = family(h, refusal);
        if (rc) return rc;
    }
    h->*slot = (Fn)fn;
    return CLIK_OK;
}
// ... the summary kernel comes with its work-size function
template <class H>
static int attach_summary_kernel(H* h, void* fn, void* work_bytes_fn, int (*family)(H*, const char*), const char* refusal)
{
    if (h && fn) {
        CLIK_NEEDS_DEVICE_HANDLE(h);
        if (!work_bytes_fn) return fail(CLIK_EINVAL, "the summary kernel comes with its work-size function");
    }
    const int rc = attach_on_demand(h, &clik_handle::summary_fn, fn, family, refusal);
    if (rc) return rc;
    h->summary_work_fn = fn ? (clik_summary_work_fn)work_bytes_fn : nullptr;
    return CLIK_OK;
}

extern "C" int clik_pinv_attach_rec_kernel(clik_pinv* h, void* rollout_rec_fn, void* value_rollout_rec_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);        // (also when detaching, unlike the others)
    const int rc = attach_on_demand(h, &clik_pinv::rec_rollout, rollout_rec_fn, pinv_attach_checks,
                                    "recording rollouts exist for skills a shape-specialised kernel serves");
    if (rc) return rc;
    h->val_rec_rollout = (clik_jit_rollout_fn)value_rollout_rec_fn;
    return CLIK_OK;
}
extern "C" int clik_qp_attach_rec_kernel(clik_qp* h, void* rollout_rec_fn, void* value_rollout_rec_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);        // (also when detaching, unlike the others)
    const int rc = attach_on_demand(h, &clik_qp::rec_rollout, rollout_rec_fn, qp_attach_checks, kQpFamily);
    if (rc) return rc;
    // (the value-specialised rollout exists for the box family only)
    h->val_rec_rollout = CLIK_QP_BOX_OK(h->host.shape) ? (clik_qp_value_rec_fn)value_rollout_rec_fn : nullptr;
    return CLIK_OK;
}
extern "C" int clik_pinv_attach_monitor_kernel(clik_pinv* h, void* fn)
{
    return attach_on_demand(h, &clik_handle::monitor_fn, fn, pinv_attach_checks,
                            "constraint values exist for skills a shape-specialised kernel serves");
}
extern "C" int clik_qp_attach_monitor_kernel(clik_qp* h, void* fn)
{
    return attach_on_demand(h, &clik_handle::monitor_fn, fn, qp_attach_checks, kQpFamily);
}
extern "C" int clik_pinv_attach_summary_kernel(clik_pinv* h, void* fn, void* work_bytes_fn)
{
    return attach_summary_kernel(h, fn, work_bytes_fn, pinv_attach_checks,
                                 "constraint summaries exist for skills a shape-specialised kernel serves");
}
extern "C" int clik_qp_attach_summary_kernel(clik_qp* h, void* fn, void* work_bytes_fn)
{
    return attach_summary_kernel(h, fn, work_bytes_fn, qp_attach_checks, kQpFamily);
}
extern "C" int clik_pinv_attach_rollout_summary_kernel(clik_pinv* h, void* fn)
{
    return attach_on_demand(h, &clik_pinv::rollsum_fn, fn, pinv_attach_checks,
                            "summarising rollouts exist for skills a shape-specialised kernel serves");
}
extern "C" int clik_qp_attach_rollout_summary_kernel(clik_qp* h, void* fn)
{
    return attach_on_demand(h, &clik_qp::rollsum_fn, fn, qp_attach_checks, kQpFamily);
}
extern "C" int clik_pinv_attach_converge_kernel(clik_pinv* h, void* fn)
{
    return attach_on_demand(h, &clik_pinv::converge_fn, fn, pinv_attach_checks,
                            "converging rollouts exist for skills a shape-specialised kernel serves");
}
extern "C" int clik_qp_attach_converge_kernel(clik_qp* h, void* fn)
{
    return attach_on_demand(h, &clik_qp::converge_fn, fn, qp_attach_checks, kQpFamily);
}

// ---- constraint values over a trajectory (clik_*_constraint_values; the kernel: clik_monitor.hpp) ---------------------
static int n_constraint_rows(const DevSkill& S)
{
    int m = 0;
    for (int ti = 0; ti < S.d.n_tasks; ++ti) m += S.d.tasks[ti].m;
    return m;
}

// the checks clik_*_constraint_values and clik_*_constraint_summary end with: the blocks the skill reads, the strides, the
// time-term table
static int trajectory_inputs_check(const DevSkill& S, const double* tterms, int64_t tt_rec_stride, int64_t tt_inst_stride,
                                   const double* x, const double* y, int64_t y_stride)
{
    if (S.d.n_x > 0 && !x) return fail(CLIK_EINVAL, "skill has virtual_var: x required");
    if (S.d.n_y > 0 && !y) return fail(CLIK_EINVAL, "skill has input_var: y required");
    if (y_stride < 0 || tt_rec_stride < 0 || tt_inst_stride < 0) return fail(CLIK_EINVAL, "negative stride");
    if (S.d.n_tslots > 0 && !tterms) return fail(CLIK_EINVAL, "tterms (device) required: the skill has time slots");
    return CLIK_OK;
}

static int constraint_values(const clik_handle* h, int64_t n_rec, int64_t B, const double* tterms, int64_t tt_rec_stride,
                             int64_t tt_inst_stride, const double* q, const double* x, const double* y, int64_t y_stride,
                             double* e, double* J, double* et, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (n_rec < 0 || B < 0) return fail(CLIK_EINVAL, "negative size");
    if (n_rec == 0 || B == 0) return CLIK_OK;
    if (!q) return fail(CLIK_EINVAL, "q must be a device pointer");
    if (!e && !J && !et) return fail(CLIK_EINVAL, "nothing to compute: e, J and et are all null");
    if (!h->monitor_fn)
        return fail(CLIK_EUNSUPPORTED, "no constraint-value kernel instantiated for this skill (clik_*_attach_monitor_kernel: "
                                       "skills of the shape-specialised family have one)");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (!h->d_img) return fail(CLIK_EUNSUPPORTED, "no skill image on the device");
    const DevSkill& S = h->host;
    const int rc = trajectory_inputs_check(S, tterms, tt_rec_stride, tt_inst_stride, x, y, y_stride);
    if (rc) return rc;
    const hipError_t er = h->monitor_fn(h->d_img, (long long)n_rec, (long long)B, S.d.n_tslots > 0 ? tterms : nullptr,
                                        (long long)tt_rec_stride, (long long)tt_inst_stride, q, x, y, (long long)y_stride, e,
                                        J, et, (hipStream_t)stream);
    if (er != hipSuccess) return hipfail(er, "constraint-value kernel launch");
    return CLIK_OK;
}

extern "C" int clik_pinv_n_constraint_rows(const clik_pinv* h) { return h ? n_constraint_rows(h->host) : 0; }
extern "C" int clik_qp_n_constraint_rows(const clik_qp* h) { return h ? n_constraint_rows(h->host) : 0; }
extern "C" int clik_pinv_constraint_values(const clik_pinv* h, int64_t n_rec, int64_t B, const double* tterms,
                                           int64_t tt_rec_stride, int64_t tt_inst_stride, const double* q, const double* x,
                                           const double* y, int64_t y_stride, double* e, double* J, double* et, void* stream)
{
    return constraint_values(h, n_rec, B, tterms, tt_rec_stride, tt_inst_stride, q, x, y, y_stride, e, J, et, stream);
}
extern "C" int clik_qp_constraint_values(const clik_qp* h, int64_t n_rec, int64_t B, const double* tterms,
                                         int64_t tt_rec_stride, int64_t tt_inst_stride, const double* q, const double* x,
                                         const double* y, int64_t y_stride, double* e, double* J, double* et, void* stream)
{
    return constraint_values(h, n_rec, B, tterms, tt_rec_stride, tt_inst_stride, q, x, y, y_stride, e, J, et, stream);
}

// ---- constraint summaries over a trajectory (clik_*_constraint_summary; the kernels: clik_summary.hpp) -----------------
// tol and the seven outputs of a summary (all device), as the entry points of the summaries and of the summarising rollouts
// take them one by one: filled once there, in the order the attached functions take them
struct SummaryIo {
    const double* tol;
    double* abs_max; int32_t* abs_max_at; double* last; double* rms; double* viol_max; int32_t* viol_count;
    int32_t* settled_at;
};

static int summary_io_check(const SummaryIo& o)
{
    if (!o.abs_max || !o.abs_max_at || !o.last || !o.rms || !o.viol_max || !o.viol_count)
        return fail(CLIK_EINVAL, "abs_max, abs_max_at, last, rms, viol_max and viol_count must be device pointers");
    if ((o.tol == nullptr) != (o.settled_at == nullptr)) return fail(CLIK_EINVAL, "tol and settled_at go together");
    return CLIK_OK;
}

static int constraint_summary(const clik_handle* h, int64_t n_rec, int64_t B, const double* tterms, int64_t tt_rec_stride,
                              int64_t tt_inst_stride, const double* q, const double* x, const double* y, int64_t y_stride,
                              void* work, int64_t work_bytes, const SummaryIo& o, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (n_rec < 0 || B < 0) return fail(CLIK_EINVAL, "negative size");
    if (n_rec == 0 || B == 0) return CLIK_OK;
    if (!q) return fail(CLIK_EINVAL, "q must be a device pointer");
    int rc = summary_io_check(o);
    if (rc) return rc;
    if (!h->summary_fn || !h->summary_work_fn)
        return fail(CLIK_EUNSUPPORTED, "no constraint-summary kernel instantiated for this skill (clik_*_attach_summary_kernel: "
                                       "skills of the shape-specialised family have one)");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (!h->d_img) return fail(CLIK_EUNSUPPORTED, "no skill image on the device");
    if (n_rec > 0x7fffffffLL) return fail(CLIK_EINVAL, "more than 2^31 - 1 records");
    const DevSkill& S = h->host;
    rc = trajectory_inputs_check(S, tterms, tt_rec_stride, tt_inst_stride, x, y, y_stride);
    if (rc) return rc;
    const unsigned long long need = h->summary_work_fn((long long)n_rec, (long long)B);
    if (!work || work_bytes < 0 || (unsigned long long)work_bytes < need)
        return fail(CLIK_EINVAL, "work must hold %llu bytes (clik_*_summary_work_bytes), got %lld", need, (long long)work_bytes);
    const hipError_t er = h->summary_fn(h->d_img, (long long)n_rec, (long long)B, S.d.n_tslots > 0 ? tterms : nullptr,
                                        (long long)tt_rec_stride, (long long)tt_inst_stride, q, x, y, (long long)y_stride,
                                        o.tol, work, (unsigned long long)work_bytes, o.abs_max, o.abs_max_at, o.last, o.rms,
                                        o.viol_max, o.viol_count, o.settled_at, (hipStream_t)stream);
    if (er != hipSuccess) return hipfail(er, "constraint-summary kernel launch");
    return CLIK_OK;
}

static int64_t summary_work_bytes(const clik_handle* h, int64_t n_rec, int64_t B)
{
    if (!h || !h->summary_work_fn || n_rec <= 0 || B <= 0) return 0;
    return (int64_t)h->summary_work_fn((long long)n_rec, (long long)B);
}

extern "C" int64_t clik_summary_chunk_length(int64_t n_rec, int64_t B)
{
    // (clik_summary.hpp: summary_chunk_length - restated, because this unit holds entry points and no kernel header;
    // tests/test_summary_codegen.py holds this, the header's and jit.summary_chunk_length together)
    const int64_t groups = B > 0 ? (B + 255) / 256 : 1;
    const int64_t want = groups < 1024 ? 1024 / groups : 1;
    const int64_t c = (n_rec + want - 1) / want;
    return c > 8 ? c : 8;
}

extern "C" int64_t clik_pinv_summary_work_bytes(const clik_pinv* h, int64_t n_rec, int64_t B)
{
    return summary_work_bytes(h, n_rec, B);
}
extern "C" int64_t clik_qp_summary_work_bytes(const clik_qp* h, int64_t n_rec, int64_t B)
{
    return summary_work_bytes(h, n_rec, B);
}
extern "C" int clik_pinv_constraint_summary(const clik_pinv* h, int64_t n_rec, int64_t B, const double* tterms,
                                            int64_t tt_rec_stride, int64_t tt_inst_stride, const double* q, const double* x,
                                            const double* y, int64_t y_stride, const double* tol, void* work,
                                            int64_t work_bytes, double* abs_max, int32_t* abs_max_at, double* last,
                                            double* rms, double* viol_max, int32_t* viol_count, int32_t* settled_at,
                                            void* stream)
{
    return constraint_summary(h, n_rec, B, tterms, tt_rec_stride, tt_inst_stride, q, x, y, y_stride, work, work_bytes,
                              {tol, abs_max, abs_max_at, last, rms, viol_max, viol_count, settled_at}, stream);
}
extern "C" int clik_qp_constraint_summary(const clik_qp* h, int64_t n_rec, int64_t B, const double* tterms,
                                          int64_t tt_rec_stride, int64_t tt_inst_stride, const double* q, const double* x,
                                          const double* y, int64_t y_stride, const double* tol, void* work,
                                          int64_t work_bytes, double* abs_max, int32_t* abs_max_at, double* last, double* rms,
                                          double* viol_max, int32_t* viol_count, int32_t* settled_at, void* stream)
{
    return constraint_summary(h, n_rec, B, tterms, tt_rec_stride, tt_inst_stride, q, x, y, y_stride, work, work_bytes,
                              {tol, abs_max, abs_max_at, last, rms, viol_max, viol_count, settled_at}, stream);
}

static int pinv_rollout_common(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                               double max_speed, const TtSource& tts, double* q, double* x, const double* y,
                               double* dq, double* dx, int32_t* mode, void* stream, const clik::RollRec* rec)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (B < 0 || n_ticks < 0) return fail(CLIK_EINVAL, "negative size");
    int stages = 1;
    int rc = stages_of(method, &stages);
    if (rc) return rc;
    if (B == 0 || n_ticks == 0) return CLIK_OK;
    const DevSkill& S = h->host;
    const bool has_static = pinv_shape_served(h);
    rc = virtual_var_check(S, x, dx, " (clik_pinv_rollout_batch_x)");
    if (rc) return rc;
    if (S.d.n_x > 0 && !has_static)
        return fail(CLIK_EUNSUPPORTED, "the rollout of a skill with virtual_var needs a shape-specialised kernel "
                                       "(none attached for this skill)");
    if (method == CLIK_INTEGRATE_RK4 && !has_static)
        return fail(CLIK_EUNSUPPORTED, "the Runge-Kutta rollout needs a shape-specialised kernel (none attached for this skill)");
    if (!has_static && skill_needs_static(S))
        return extern_needs_kernel("clik_pinv_rollout_batch");
    if (h->kernel < 0 && !h->jit_rollout) return no_kernel_for_wide_state(S, "clik_pinv_rollout_batch");
    rc = joint_args_check(S, q, y, dq);
    if (rc) return rc;
    if (rec && !h->rec_rollout)
        return fail(CLIK_EUNSUPPORTED, "records and per-tick targets need a shape-specialised recording rollout (none "
                                       "attached for this skill: clik_pinv_attach_rec_kernel)");
    TtBuffer tt;
    rc = rollout_tterms(tts, S.d.n_tslots, n_ticks, stages, dt, (hipStream_t)stream, &tt);
    if (rc) return rc;
    double* const d_tt = tt.ptr;
    const clik::LaunchArgs la = launch_args(h, x, dx, stages, nullptr, rec);
    hipError_t e = hipErrorNotSupported;
    if (rec) {
        if (h->val_rec_rollout && h->val_rollout && S.d.n_x == 0 &&
            clik::pinv_value_variant(clik::pinv_select(S.shape, h->policy, (long long)B, clik::PinvOp::rollout)))
            e = h->val_rec_rollout(&la, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, mode, (hipStream_t)stream);
        if (e == hipErrorNotSupported)
            e = h->rec_rollout(&la, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, mode, (hipStream_t)stream);
        if (e != hipSuccess) return hipfail(e, "pinv recording rollout launch");
        return CLIK_OK;
    }
    if (h->val_rollout && S.d.n_x == 0 &&
        clik::pinv_value_variant(clik::pinv_select(S.shape, h->policy, (long long)B, clik::PinvOp::rollout)))
        e = h->val_rollout(&la, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, mode, (hipStream_t)stream);
    if (e == hipErrorNotSupported)          // (see pinv_solve_common)
        e = h->jit_rollout
                ? h->jit_rollout(&la, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, mode,
                                 (hipStream_t)stream)
                : clik::pinv_launch_rollout(h->kernel, la, d_tt, n_ticks, dt, max_speed, (long long)B,
                                            q, y, dq, mode, (hipStream_t)stream);
    if (e != hipSuccess) return hipfail(e, "pinv_rollout_kernel launch");
    return CLIK_OK;
}

// ---- rollouts that summarise their constraint values while they run (clik_*_rollout_batch_sum; the kernels:
// clik_rollout_summary.hpp) --------------------------------------------------------------------------------------------
// what both controllers check before anything else: sizes, the outputs, and where the tick times come from
static int rollout_sum_checks(int64_t B, int32_t n_ticks, int32_t method, int n_tslots, const double* tterms,
                              const double* times, const SummaryIo& o, int* stages)
{
    if (B < 0) return fail(CLIK_EINVAL, "negative size");
    if (n_ticks < 1) return fail(CLIK_EINVAL, "a summarising rollout needs at least one tick, got %d", n_ticks);
    int rc = stages_of(method, stages);
    if (rc) return rc;
    rc = summary_io_check(o);
    if (rc) return rc;
    if (tterms && times) return fail(CLIK_EINVAL, "tterms (host) and times (device) are alternatives: pass one");
    if (n_tslots > 0 && !tterms && !times)
        return fail(CLIK_EINVAL, "the skill has time slots: tterms (host) or times (device) required");
    return CLIK_OK;
}

extern "C" int clik_pinv_rollout_batch_sum(const clik_pinv* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                           double max_speed, const double* tterms, double* q, double* x,
                                           const double* y, double* dq, double* dx, int32_t* mode, void* stream,
                                           int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                           double* rec_x, double* rec_dx, int32_t* rec_mode, const double* times,
                                           const double* tol, double* abs_max, int32_t* abs_max_at, double* last,
                                           double* rms, double* viol_max, int32_t* viol_count, int32_t* settled_at)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    const DevSkill& S = h->host;
    const SummaryIo o = {tol, abs_max, abs_max_at, last, rms, viol_max, viol_count, settled_at};
    int stages = 1;
    int rc = rollout_sum_checks(B, n_ticks, method, S.d.n_tslots, tterms, times, o, &stages);
    if (rc) return rc;
    clik::RollRec rr;
    rc = roll_rec_of(B, S.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, nullptr, rec_mode, &rr);
    if (rc) return rc;
    if (B == 0) return CLIK_OK;
    if (!h->rollsum_fn)
        return fail(CLIK_EUNSUPPORTED, "no summarising rollout instantiated for this skill "
                                       "(clik_pinv_attach_rollout_summary_kernel: skills of the shape-specialised family have one)");
    rc = virtual_var_check(S, x, dx);
    if (rc) return rc;
    // (as clik_pinv_rollout_batch_m: a skill whose rollouts are the built-in kernel's has no Runge-Kutta rollout, with or
    // without a summary)
    if (method == CLIK_INTEGRATE_RK4 && !pinv_shape_served(h))
        return fail(CLIK_EUNSUPPORTED, "the Runge-Kutta rollout needs a shape-specialised kernel (none attached for this skill)");
    rc = joint_args_check(S, q, y, dq);
    if (rc) return rc;
    TtBuffer tt;
    rc = rollout_tterms(times ? tt_device(times, h->time_fn) : tt_host(tterms), S.d.n_tslots, n_ticks, stages, dt,
                        (hipStream_t)stream, &tt);
    if (rc) return rc;
    const clik::LaunchArgs la = launch_args(h, x, dx, stages, nullptr, &rr);
    const hipError_t e = h->rollsum_fn(&la, tt.ptr, n_ticks, dt, max_speed, (long long)B, q, y, dq, mode, (hipStream_t)stream,
                                       o.tol, o.abs_max, o.abs_max_at, o.last, o.rms, o.viol_max, o.viol_count, o.settled_at);
    if (e != hipSuccess) return hipfail(e, "pinv summarising rollout launch");
    return CLIK_OK;
}

// ---- rollouts that run until each instance has converged (clik_*_converge_batch; the kernels: clik_converge.hpp) --------
// what both controllers check before anything else
static int converge_checks(int64_t B, int32_t max_ticks, const double* tol, const int32_t* ticks,
                           const int32_t* stop_status, const double* residual)
{
    if (B < 1) return fail(CLIK_EINVAL, "a converging rollout needs at least one instance, got %lld", (long long)B);
    if (max_ticks < 0) return fail(CLIK_EINVAL, "max_ticks must be >= 0, got %d", max_ticks);
    if (!tol) return fail(CLIK_EINVAL, "tol (device, one value per constraint row) required");
    if (!ticks || !stop_status || !residual)
        return fail(CLIK_EINVAL, "ticks, stop_status and residual must be device pointers");
    return CLIK_OK;
}

extern "C" int clik_pinv_converge_batch(const clik_pinv* h, int64_t B, int32_t max_ticks, double dt, double max_speed,
                                        double min_step, const double* tterms, double* q, double* x, const double* y,
                                        double* dq, double* dx, int32_t* mode, const double* tol, int32_t* ticks,
                                        int32_t* stop_status, double* residual, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    const DevSkill& S = h->host;
    int rc = converge_checks(B, max_ticks, tol, ticks, stop_status, residual);
    if (rc) return rc;
    if (!h->converge_fn)
        return fail(CLIK_EUNSUPPORTED, "no converging rollout instantiated for this skill "
                                       "(clik_pinv_attach_converge_kernel: skills of the shape-specialised family have one)");
    rc = state_args_check(S, q, x, y, dq, dx);
    if (rc) return rc;
    TickArgs tk;
    rc = fill_tick(S, tterms, &tk);
    if (rc) return rc;
    const clik::LaunchArgs la = launch_args(h, x, dx, 1, nullptr, nullptr);
    const hipError_t e = h->converge_fn(&la, &tk, (long long)B, max_ticks, dt, max_speed, min_step, q, y, dq, mode,
                                        (hipStream_t)stream, tol, ticks, stop_status, residual);
    if (e != hipSuccess) return hipfail(e, "pinv converging rollout launch");
    return CLIK_OK;
}

// ---------------------------------------------------------------------------- QP
static int qp_upload_image(clik_qp* h)
{
    if (h->d_img) return CLIK_OK;
    std::vector<char> img;
    if (!build_qp_image(h->host, img))
        return fail(CLIK_EUNSUPPORTED, "skill rows are not contiguous: no static kernel possible");
    const hipError_t e = upload_image(h, img);
    if (e != hipSuccess) return hipfail(e, "QP skill image upload");
    return CLIK_OK;
}

static int qp_attach_checks(clik_qp* h, const char* refusal)
{
    if (!qp_static_eligible(h->host)) return fail(CLIK_EUNSUPPORTED, "%s", refusal);
    return qp_upload_image(h);
}

extern "C" int clik_qp_create(const clik_skill_desc* desc, const clik_qp_opts* opts, clik_qp** out)
{
    if (!out) return fail(CLIK_EINVAL, "null out pointer");
    *out = nullptr;
    if (!opts) return fail(CLIK_EINVAL, "null options");
    std::unique_ptr<clik_qp> h(new (std::nothrow) clik_qp());
    if (!h) return fail(CLIK_ENOMEM, "out of host memory");
    h->gws.reset(new (std::nothrow) clik::GwsOwner());
    if (!h->gws) return fail(CLIK_ENOMEM, "out of host memory");
    int used_rows = 0;
    int rc = validate_and_derive(desc, &h->host, &used_rows);
    if (rc) return rc;
    DevSkill& S = h->host;
    S.qo = *opts;
    if (S.qo.max_iter <= 0) S.qo.max_iter = 4 * (S.n_qp_rows + S.n_qp_vars) + 16;
    for (int k = 0; k < S.n_slack; ++k)
        if (!(opts->weight_shifter + opts->slack_weights[k] > 0.0))
            return fail(CLIK_EINVAL, "QP slack weight %d makes the cost non-convex", k);
    if (S.n_qp_vars > CLIK_MAX_QPVARS || S.n_qp_rows > CLIK_MAX_QPROWS)
        return fail(CLIK_EUNSUPPORTED, "QP with %d variables x %d rows exceeds the device limits (%d x %d)",
                    S.n_qp_vars, S.n_qp_rows, CLIK_MAX_QPVARS, CLIK_MAX_QPROWS);
    for (int j = 0; j < S.n; ++j)
        if (!(opts->weight_shifter * opts->state_weights[j] > 0.0))
            return fail(CLIK_EINVAL, "QP cost weight %d is not positive", j);
    {
        int need = S.n;
        for (int ti = 0; ti < S.d.n_tasks; ++ti)
            if (S.d.tasks[ti].m > need) need = S.d.tasks[ti].m;
        h->variant = clik::qp_pick_variant(need, S.n_qp_vars, S.n_qp_rows);
    }
    finish_qp_shape(S);
    const bool eligible = qp_static_eligible(S);
    {
        // The built-in (dynamic) kernel keeps every row, soft equalities included, in its active set;
        // the shape-specialised kernels eliminate those and fit larger skills.  A skill only they can
        // serve gets a handle without a built-in kernel (variant -1): it solves once a kernel is
        // attached (clik_qp_attach_kernel) or the AOT table has one.
        const bool dyn_rows = h->variant >= 0;
        const bool dyn_lds = dyn_rows && clik::qp_variant_lds(h->variant, S.d.n_y) <= clik::kLdsBytesPerCu;
        if (!dyn_lds) {
            if (!eligible) {
                if (!dyn_rows)
                    return fail(CLIK_EUNSUPPORTED,
                                "no QP kernel variant for %d variables x %d rows (device limit: %d rows)",
                                S.n_qp_vars, S.n_qp_rows, CLIK_MAX_QPROWS);
                return fail(CLIK_EUNSUPPORTED, "QP needs more LDS than a CU has (input_var too large)");
            }
            h->variant = -1;
        }
    }
    compute_warm(S, used_rows, h->warm);
    S.lds_slots = 0;        // (the QP kernels size their LDS themselves)
    {
        // the switches of the kernel choice (qp_select, clik_qp_select.hpp): CLIK_FORCE_DYNAMIC=1 / CLIK_NO_AOT=1 skip
        // the AOT table (the Python layer may still attach a run-time instantiated kernel)
        const char* force = getenv("CLIK_FORCE_DYNAMIC");
        const char* noaot = getenv("CLIK_NO_AOT");
        h->policy.aot = !((force && force[0] == '1') || (noaot && noaot[0] == '1'));
        h->policy.folio = clik::qp_env().folio;
    }
    // shape-specialised kernel from the AOT table (a host-only handle picks it too, and uploads nothing)
    h->static_k = (h->policy.aot && eligible) ? clik::qp_pick_static(S.shape) : -1;
    rc = upload_skill(h.get());
    if (rc) return rc;
    if (h->dev) {
        if (h->static_k >= 0) {
            rc = qp_upload_image(h.get());
            if (rc) return rc;
        }
        h->policy.cus = clik::current_device_cus();
    }
    *out = h.release();
    return CLIK_OK;
}

// what the handle holds, as qp_select sees it
static clik::QpKernels qp_kernels(const clik_qp* h)
{
    clik::QpKernels k;
    k.aot = h->static_k >= 0;
    k.jit_solve = h->jit_solve != nullptr;
    k.jit_rollout = h->jit_rollout != nullptr;
    k.value_rollout = h->val_rollout != nullptr;
    k.dyn_width = clik::qp_variant_width(h->variant);
    k.generated = skill_has_extern(h->host);
    k.wide = skill_has_wide_task(h->host);
    return k;
}

// a shape-specialised kernel (AOT or attached) serves the handle's ticks: what a value-specialised one stands in for
static bool qp_shape_served(const clik_qp* h)
{
    clik::QpPolicy image = h->policy;
    image.values_attached = false;
    return clik::qp_shape_kernel(clik::qp_select(h->host.shape, image, qp_kernels(h), 1, false, clik::QpOp::tick));
}

// ShapeDesc initialiser of a QP skill (see clik_shape_describe); returns 1 when a
// shape-specialised QP kernel can serve it, 0 when not, negative on error.
extern "C" int clik_qp_shape_describe(const clik_skill_desc* desc, char* buf, int cap)
{
    if (!buf || cap <= 0) return fail(CLIK_EINVAL, "bad arguments");
    std::unique_ptr<DevSkill> S(new (std::nothrow) DevSkill());
    if (!S) return fail(CLIK_ENOMEM, "out of host memory");
    int rc = validate_and_derive(desc, S.get());
    if (rc) return rc;
    finish_qp_shape(*S);
    const std::string o = shape_to_string(S->shape);
    const bool eligible = qp_static_eligible(*S);
    if ((int)o.size() + 1 > cap) return fail(CLIK_EINVAL, "buffer too small");
    memcpy(buf, o.c_str(), o.size() + 1);
    return eligible ? 1 : 0;
}

// Attach a shape-specialised QP kernel compiled at run time (casclik_amd/jit.py instantiates
// clik_qp_static.hpp for the ShapeDesc that clik_qp_shape_describe printed).
extern "C" int clik_qp_attach_kernel(clik_qp* h, void* solve_fn, void* rollout_fn, const char* name)
{
    // (rollout_fn may be NULL: clik_qp_rollout_batch then needs an AOT kernel)
    if (!h || !solve_fn) return fail(CLIK_EINVAL, "null argument");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (!qp_static_eligible(h->host))
        return fail(CLIK_EUNSUPPORTED, "skill is outside the shape-specialised QP family");
    int rc = qp_upload_image(h);
    if (rc) return rc;
    h->jit_solve = (clik::qp_jit_fn)solve_fn;
    h->jit_rollout = (clik::qp_static_rollout_fn)rollout_fn;
    snprintf(h->jit_name, sizeof(h->jit_name), "%s", name ? name : "jit");
    return CLIK_OK;
}

// n_ticks of QP solve -> clamp -> Euler in one launch (SURVEY.md 8(f).1 for the QP controller); the
// working set is carried from tick to tick inside the kernel.  Needs a shape-specialised kernel.
extern "C" int clik_qp_rollout_batch(const clik_qp* hc, int64_t B, int32_t n_ticks, double dt, double max_speed,
                                     const double* tterms, double* q, const double* y, double* dq,
                                     double* slack, int32_t* status, void* stream)
{
    return clik_qp_rollout_batch_x(hc, B, n_ticks, dt, max_speed, tterms, q, nullptr, y, dq, nullptr, slack, status,
                                   stream);
}

extern "C" int clik_qp_rollout_batch_x(const clik_qp* hc, int64_t B, int32_t n_ticks, double dt, double max_speed,
                                       const double* tterms, double* q, double* x, const double* y, double* dq,
                                       double* dx, double* slack, int32_t* status, void* stream)
{
    return clik_qp_rollout_batch_m(hc, B, n_ticks, CLIK_INTEGRATE_EULER, dt, max_speed, tterms, q, x, y, dq, dx, slack,
                                   status, stream);
}

static int qp_rollout_common(const clik_qp* hc, int64_t B, int32_t n_ticks, int32_t method, double dt,
                             double max_speed, const TtSource& tts, double* q, double* x, const double* y,
                             double* dq, double* dx, double* slack, int32_t* status, void* stream,
                             const clik::RollRec* rec);

extern "C" int clik_qp_rollout_batch_m(const clik_qp* hc, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                       double max_speed, const double* tterms, double* q, double* x, const double* y,
                                       double* dq, double* dx, double* slack, int32_t* status, void* stream)
{
    return qp_rollout_common(hc, B, n_ticks, method, dt, max_speed, tt_host(tterms), q, x, y, dq, dx, slack, status, stream,
                             nullptr);
}

extern "C" int clik_qp_rollout_batch_rec(const clik_qp* hc, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                         double max_speed, const double* tterms, double* q, double* x, const double* y,
                                         double* dq, double* dx, double* slack, int32_t* status, void* stream,
                                         int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                         double* rec_x, double* rec_dx, double* rec_slack, int32_t* rec_status)
{
    if (!hc) return fail(CLIK_EINVAL, "null handle");
    clik::RollRec rr;
    int rc = roll_rec_of(B, hc->host.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, rec_slack, rec_status,
                         &rr);
    if (rc) return rc;
    return qp_rollout_common(hc, B, n_ticks, method, dt, max_speed, tt_host(tterms), q, x, y, dq, dx, slack, status, stream,
                             &rr);
}

extern "C" int clik_qp_rollout_batch_dev(const clik_qp* hc, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                         double max_speed, const double* times, double* q, double* x, const double* y,
                                         double* dq, double* dx, double* slack, int32_t* status, void* stream,
                                         int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                         double* rec_x, double* rec_dx, double* rec_slack, int32_t* rec_status)
{
    if (!hc) return fail(CLIK_EINVAL, "null handle");
    const TtSource tts = tt_device(times, hc->time_fn);
    if (record_every == 0 && y_per_tick == 0)
        return qp_rollout_common(hc, B, n_ticks, method, dt, max_speed, tts, q, x, y, dq, dx, slack, status, stream, nullptr);
    clik::RollRec rr;
    int rc = roll_rec_of(B, hc->host.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, rec_slack, rec_status,
                         &rr);
    if (rc) return rc;
    return qp_rollout_common(hc, B, n_ticks, method, dt, max_speed, tts, q, x, y, dq, dx, slack, status, stream, &rr);
}

static int qp_rollout_common(const clik_qp* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                             double max_speed, const TtSource& tts, double* q, double* x, const double* y,
                             double* dq, double* dx, double* slack, int32_t* status, void* stream,
                             const clik::RollRec* rec)
{
    int stages = 1;
    int rc = stages_of(method, &stages, "clik_qp_rollout_batch_m: ");
    if (rc) return rc;
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (B < 0 || n_ticks < 0) return fail(CLIK_EINVAL, "negative size");
    if (B == 0 || n_ticks == 0) return CLIK_OK;
    const DevSkill& S = h->host;
    rc = virtual_var_check(S, x, dx, " (clik_qp_rollout_batch_x)");
    if (rc) return rc;
    const clik::QpKernel k = clik::qp_select(S.shape, h->policy, qp_kernels(h), (long long)B, false, clik::QpOp::rollout);
    if (k == clik::QpKernel::none)
        return fail(CLIK_EUNSUPPORTED, "the QP rollout needs a shape-specialised kernel (none attached for this skill)");
    rc = joint_args_check(S, q, y, dq);
    if (rc) return rc;
    if (rec && !h->rec_rollout)
        return fail(CLIK_EUNSUPPORTED, "records and per-tick targets need a shape-specialised recording rollout (none "
                                       "attached for this skill: clik_qp_attach_rec_kernel)");
    TtBuffer tt;
    rc = rollout_tterms(tts, S.d.n_tslots, n_ticks, stages, dt, (hipStream_t)stream, &tt);
    if (rc) return rc;
    double* const d_tt = tt.ptr;
    if (rec) {
        hipError_t er = (k == clik::QpKernel::value && h->val_rec_rollout)
                            ? h->val_rec_rollout(d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, slack, status, x, dx,
                                                 (hipStream_t)stream, stages, rec)
                            : h->rec_rollout(h->d_img, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, slack, status,
                                             x, dx, (hipStream_t)stream, stages, rec);
        if (er != hipSuccess) return hipfail(er, "qp recording rollout launch");
        return CLIK_OK;
    }
    hipError_t e = k == clik::QpKernel::value
                       ? h->val_rollout(d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, slack, status, x, dx,
                                        (hipStream_t)stream, stages)
                   : k == clik::QpKernel::jit
                       ? h->jit_rollout(h->d_img, d_tt, n_ticks, dt, max_speed, (long long)B, q, y, dq, slack,
                                        status, x, dx, (hipStream_t)stream, stages)
                       : clik::qp_launch_rollout_static(h->static_k, h->d_img, d_tt, n_ticks, dt, max_speed,
                                                        (long long)B, q, y, dq, slack, status, x, dx,
                                                        (hipStream_t)stream, stages);
    if (e != hipSuccess) return hipfail(e, "qp_rollout_kernel launch");
    return CLIK_OK;
}

extern "C" int clik_qp_rollout_batch_sum(const clik_qp* h, int64_t B, int32_t n_ticks, int32_t method, double dt,
                                         double max_speed, const double* tterms, double* q, double* x, const double* y,
                                         double* dq, double* dx, double* slack, int32_t* status, void* stream,
                                         int32_t y_per_tick, int32_t record_every, double* rec_q, double* rec_dq,
                                         double* rec_x, double* rec_dx, double* rec_slack, int32_t* rec_status,
                                         const double* times, const double* tol, double* abs_max, int32_t* abs_max_at,
                                         double* last, double* rms, double* viol_max, int32_t* viol_count,
                                         int32_t* settled_at)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    const DevSkill& S = h->host;
    const SummaryIo o = {tol, abs_max, abs_max_at, last, rms, viol_max, viol_count, settled_at};
    int stages = 1;
    int rc = rollout_sum_checks(B, n_ticks, method, S.d.n_tslots, tterms, times, o, &stages);
    if (rc) return rc;
    clik::RollRec rr;
    rc = roll_rec_of(B, S.d.n_y, y_per_tick, record_every, rec_q, rec_dq, rec_x, rec_dx, rec_slack, rec_status, &rr);
    if (rc) return rc;
    if (B == 0) return CLIK_OK;
    if (!h->rollsum_fn || !h->d_img)
        return fail(CLIK_EUNSUPPORTED, "no summarising rollout instantiated for this skill "
                                       "(clik_qp_attach_rollout_summary_kernel: skills of the shape-specialised family have one)");
    rc = state_args_check(S, q, x, y, dq, dx);
    if (rc) return rc;
    TtBuffer tt;
    rc = rollout_tterms(times ? tt_device(times, h->time_fn) : tt_host(tterms), S.d.n_tslots, n_ticks, stages, dt,
                        (hipStream_t)stream, &tt);
    if (rc) return rc;
    const hipError_t e = h->rollsum_fn(h->d_img, tt.ptr, n_ticks, dt, max_speed, (long long)B, q, y, dq, slack, status, x, dx,
                                       (hipStream_t)stream, stages, &rr, o.tol, o.abs_max, o.abs_max_at, o.last, o.rms,
                                       o.viol_max, o.viol_count, o.settled_at);
    if (e != hipSuccess) return hipfail(e, "qp summarising rollout launch");
    return CLIK_OK;
}

extern "C" int clik_qp_converge_batch(const clik_qp* h, int64_t B, int32_t max_ticks, double dt, double max_speed,
                                      double min_step, const double* tterms, double* q, double* x, const double* y,
                                      double* dq, double* dx, int32_t* status, double* slack, const double* tol,
                                      int32_t* ticks, int32_t* stop_status, double* residual, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    const DevSkill& S = h->host;
    int rc = converge_checks(B, max_ticks, tol, ticks, stop_status, residual);
    if (rc) return rc;
    if (!h->converge_fn || !h->d_img)
        return fail(CLIK_EUNSUPPORTED, "no converging rollout instantiated for this skill "
                                       "(clik_qp_attach_converge_kernel: skills of the shape-specialised family have one)");
    rc = state_args_check(S, q, x, y, dq, dx);
    if (rc) return rc;
    TickArgs tk;
    rc = fill_tick(S, tterms, &tk);
    if (rc) return rc;
    const hipError_t e = h->converge_fn(h->d_img, &tk, (long long)B, max_ticks, dt, max_speed, min_step, q, y, dq, slack,
                                        status, x, dx, (hipStream_t)stream, tol, ticks, stop_status, residual);
    if (e != hipSuccess) return hipfail(e, "qp converging rollout launch");
    return CLIK_OK;
}

// the skill image + QP options of this handle (what the shape-specialised QP kernels read from memory, laid out
// as clik::QpImg) as 64-bit words, for casclik_amd/jit.py to compile into a value-specialised kernel
extern "C" int clik_qp_image_words(const clik_qp* h, uint64_t* buf, int cap)
{
    if (!h || !buf || cap <= 0) return fail(CLIK_EINVAL, "bad arguments");
    std::vector<char> img;
    if (!build_qp_image(h->host, img)) return fail(CLIK_EUNSUPPORTED, "skill rows are not contiguous");
    size_t image_bytes = 0;
    {
        std::vector<char> plain;
        if (!build_skill_image(h->host, plain, &image_bytes, sizeof(clik::QpTail))) return fail(CLIK_EUNSUPPORTED, "no image");
    }
    const size_t bytes = ((((image_bytes + 15) & ~(size_t)15) + sizeof(clik::QpTail)) + 15) & ~(size_t)15;
    const int words = (int)(bytes / 8);
    if (words > cap) return fail(CLIK_EINVAL, "image needs %d words, buffer holds %d", words, cap);
    memset(buf, 0, (size_t)words * 8);
    memcpy(buf, img.data(), img.size() < bytes ? img.size() : bytes);
    return words;
}

// 1: after folding the soft equalities every remaining row of the skill's QP is a hard bound on one state (the
// family solved by Gauss-Seidel sweeps + the primal active set, and the one whose value-specialised kernel needs no LDS)
extern "C" int clik_qp_is_box_family(const clik_qp* h)
{
    if (!h) return 0;
    return (qp_shape_served(h) && CLIK_QP_BOX_OK(h->host.shape)) ? 1 : 0;
}

extern "C" int clik_qp_attach_value_kernel(clik_qp* h, void* solve_fn, void* rollout_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (solve_fn && !qp_shape_served(h))
        return fail(CLIK_EUNSUPPORTED, "value-specialised QP kernels exist for skills a shape-specialised kernel serves");
    h->val_solve = (clik::qp_value_fn)solve_fn;
    // (the value-specialised rollout exists for the box family only)
    h->val_rollout = (solve_fn && CLIK_QP_BOX_OK(h->host.shape)) ? (clik::qp_value_rollout_fn)rollout_fn : nullptr;
    h->policy.values_attached = solve_fn != nullptr;
    return CLIK_OK;
}

extern "C" int clik_qp_attach_resident_kernel(clik_qp* h, void* resident_fn)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (resident_fn && !clik::qp_resident_ok(h->host.shape))
        return fail(CLIK_EUNSUPPORTED, "resident QP ticks exist for bound-constrained skills with forward kinematics and "
                                       "without virtual variables");
    h->val_resident = (decltype(h->val_resident))resident_fn;
    return CLIK_OK;
}

extern "C" int clik_qp_resident_waves(const clik_qp* h, int64_t B)
{
    if (!h || B <= 0) return fail(CLIK_EINVAL, "bad arguments");
    return (int)((B + 15) / 16);         // (four lanes per instance: one wave per 16 instances, one `done` slot per wave)
}

extern "C" int clik_qp_resident_run(const clik_qp* h, int64_t B, int32_t n_ticks, const double* tterms, const double* q,
                                    const double* y, double* dq, double* slack, int32_t* status, clik_ticket* ticket,
                                    uint32_t* done, double timeout_s, void* stream)
{
    if (!h) return fail(CLIK_EINVAL, "null handle");
    CLIK_NEEDS_DEVICE_HANDLE(h);
    TickArgs tk;
    const int rc = resident_checks(h, h->val_resident != nullptr,
                                   "resident QP ticks need the value-specialised kernel of a bound-constrained skill "
                                   "attached to this handle (none is)",
                                   B, n_ticks, tterms, q, y, dq, ticket, done, timeout_s, &tk);
    if (rc) return rc;
    const unsigned long long budget = (unsigned long long)(timeout_s * 5e6);       // (polls, at a nominal 0.2 us each)
    hipError_t e = h->val_resident(&tk, (long long)B, q, y, dq, slack, status, (void*)ticket, (unsigned*)done, n_ticks,
                                   budget, (hipStream_t)stream);
    if (e == hipErrorNotSupported)
        return fail(CLIK_EUNSUPPORTED, "resident QP ticks: %lld instances need more waves than this kernel can keep resident "
                                       "at once on this device", (long long)B);
    if (e != hipSuccess) return hipfail(e, "resident QP kernel launch");
    return CLIK_OK;
}

extern "C" const char* clik_qp_kernel_name(const clik_qp* h)
{
    if (!h) return "none";
    if (h->jit_solve) return h->jit_name;
    if (h->static_k >= 0) return clik::qp_static_name(h->static_k);
    return h->variant >= 0 ? "dynamic" : "none";
}

extern "C" const char* clik_qp_kernel_variant(const clik_qp* h, int64_t B, int32_t hot)
{
    if (!h) return "";
    return clik::kQpVariantName[(int)clik::qp_select(h->host.shape, h->policy, qp_kernels(h), (long long)B, hot != 0,
                                                     clik::QpOp::tick)];
}

extern "C" int clik_qp_destroy(clik_qp* h)
{
    delete h;       // (... and the work area of the global-workspace kernels)
    return CLIK_OK;
}

extern "C" int64_t clik_qp_workspace_bytes(const clik_qp* h) { return (h && h->gws) ? (int64_t)h->gws->footprint() : 0; }

extern "C" int clik_qp_n_vars(const clik_qp* h) { return h ? h->host.n_qp_vars : 0; }
extern "C" int clik_qp_n_rows(const clik_qp* h) { return h ? h->host.n_qp_rows : 0; }

static int qp_check_args(const clik_qp* h, int64_t B, const double* q, const double* x, const double* y)
{
    CLIK_NEEDS_DEVICE_HANDLE(h);
    if (!h) return fail(CLIK_EINVAL, "null handle");
    if (B < 0) return fail(CLIK_EINVAL, "negative batch size");
    const DevSkill& S = h->host;
    if (B > 0 && !q) return fail(CLIK_EINVAL, "q must be a device pointer");
    // (an empty batch has no rows to point at: a zero-row device tensor's data pointer is null)
    if (B > 0 && S.d.n_x > 0 && !x) return fail(CLIK_EINVAL, "skill has virtual_var: x required");
    if (B > 0 && S.d.n_y > 0 && !y) return fail(CLIK_EINVAL, "skill has input_var: y required");
    return CLIK_OK;
}

extern "C" int clik_qp_solve_batch(const clik_qp* h, int64_t B, const double* tterms, const double* q,
                                   const double* x, const double* y, double* dq, double* dx, double* slack,
                                   int32_t* status, void* stream)
{
    return clik_qp_solve_batch_hot(h, B, tterms, q, x, y, dq, dx, slack, status, nullptr, 0, stream);
}

static int qp_solve_common(const clik_qp* h, int64_t B, const double* tterms, const double* t_inst, const double* q,
                           const double* x, const double* y, double* dq, double* dx, double* slack,
                           int32_t* status, int32_t* hot_set, int32_t use_hot, void* stream)
{
    int rc = qp_check_args(h, B, q, x, y);
    if (rc) return rc;
    if (B == 0) return CLIK_OK;
    if (!dq) return fail(CLIK_EINVAL, "dq must be a device pointer");
    // (a constraint with more than eight rows is fine for the dynamic QP kernels twelve rows wide - the variant picked at
    // create time covers the widest constraint; only generated constraint code needs an instantiated kernel)
    const clik::QpKernel k = clik::qp_select(h->host.shape, h->policy, qp_kernels(h), (long long)B, use_hot != 0,
                                             t_inst ? clik::QpOp::tick_t : clik::QpOp::tick);
    if (k == clik::QpKernel::needs_instance) return extern_needs_kernel("clik_qp_solve_batch");
    TickArgs tk;
    if (t_inst == nullptr) {
        rc = fill_tick(h->host, tterms, &tk);
        if (rc) return rc;
    } else if (k == clik::QpKernel::none) {
        return fail(CLIK_EUNSUPPORTED, "clik_qp_solve_batch_t: per-instance time needs a shape-specialised kernel "
                                       "for the skill (none built in, none attached)");
    }
    hipError_t e;
    switch (k) {
    case clik::QpKernel::value_folio:
    case clik::QpKernel::value:
        e = h->val_solve(&tk, (long long)B, q, x, y, dq, dx, slack, status, hot_set, use_hot, (hipStream_t)stream);
        break;
    case clik::QpKernel::jit:
        e = h->jit_solve(h->d_img, &tk, (long long)B, q, x, y, dq, dx, slack, status, hot_set, use_hot,
                         (hipStream_t)stream, t_inst);
        break;
    case clik::QpKernel::aot:
        e = clik::qp_launch_static(h->static_k, h->d_img, tk, (long long)B, q, x, y, dq, dx, slack, status, hot_set,
                                   use_hot, (hipStream_t)stream, t_inst);
        break;
    case clik::QpKernel::dynamic:
        if (clik::qp_variant_uses_workspace(h->variant) && (hipStream_t)stream == hipStreamPerThread)
            return fail(CLIK_EUNSUPPORTED, "clik_qp_solve_batch: this skill's kernel keeps its work area in global memory, "
                                           "owned by the handle and ordered per stream - hipStreamPerThread is not supported "
                                           "for it (pass an explicit stream)");
        e = clik::qp_launch_solve(h->variant, h->dev, h->warm, tk, (long long)B, h->host.d.n_y, q, x, y, dq, dx,
                                  slack, status, (hipStream_t)stream, h->gws.get());
        if (e == hipErrorStreamCaptureUnsupported)
            return fail(CLIK_EHIP, "qp_solve_kernel launch: the work area of this skill's kernel must grow for this batch "
                                   "size, which cannot be captured - run one tick of this batch size before capturing");
        break;
    default:
        return fail(CLIK_EUNSUPPORTED, "clik_qp_solve_batch: this skill needs a shape-specialised kernel and none "
                                       "is attached (casclik_amd.jit needs hipcc)");
    }
    if (e != hipSuccess) return hipfail(e, "qp_solve_kernel launch");
    return CLIK_OK;
}

extern "C" int clik_qp_solve_batch_hot(const clik_qp* h, int64_t B, const double* tterms, const double* q,
                                       const double* x, const double* y, double* dq, double* dx, double* slack,
                                       int32_t* status, int32_t* hot_set, int32_t use_hot, void* stream)
{
    return qp_solve_common(h, B, tterms, nullptr, q, x, y, dq, dx, slack, status, hot_set, use_hot, stream);
}

extern "C" int clik_qp_solve_batch_t(const clik_qp* h, int64_t B, const double* t_inst, const double* q,
                                     const double* x, const double* y, double* dq, double* dx, double* slack,
                                     int32_t* status, int32_t* hot_set, int32_t use_hot, void* stream)
{
    if (h && h->host.d.n_tslots > 0 && !t_inst)
        return fail(CLIK_EINVAL, "clik_qp_solve_batch_t: t_inst (device, [B][2 * n_tslots]) required");
    if (h && h->host.d.n_tslots == 0)
        return qp_solve_common(h, B, nullptr, nullptr, q, x, y, dq, dx, slack, status, hot_set, use_hot, stream);
    return qp_solve_common(h, B, nullptr, t_inst, q, x, y, dq, dx, slack, status, hot_set, use_hot, stream);
}

extern "C" int clik_qp_data_batch(const clik_qp* h, int64_t B, const double* tterms, const double* q,
                                  const double* x, const double* y, double* Hdiag, double* A, double* lbA,
                                  double* ubA, void* stream)
{
    int rc = qp_check_args(h, B, q, x, y);
    if (rc) return rc;
    if (B == 0) return CLIK_OK;
    if (!Hdiag || !A || !lbA || !ubA) return fail(CLIK_EINVAL, "output pointers required");
    const clik::QpKernel k = clik::qp_select(h->host.shape, h->policy, qp_kernels(h), (long long)B, false, clik::QpOp::data);
    if (k == clik::QpKernel::needs_instance)
        return fail(CLIK_EUNSUPPORTED, "clik_qp_data_batch: not available for skills that only the "
                                       "shape-specialised kernels serve (generated rows, > 8 rows per constraint)");
    if (k == clik::QpKernel::none)
        return fail(CLIK_EUNSUPPORTED, "clik_qp_data_batch: the skill exceeds the built-in kernel's limits");
    TickArgs tk;
    rc = fill_tick(h->host, tterms, &tk);
    if (rc) return rc;
    if (clik::qp_variant_uses_workspace(h->variant) && (hipStream_t)stream == hipStreamPerThread)
        return fail(CLIK_EUNSUPPORTED, "clik_qp_data_batch: hipStreamPerThread is not supported for skills whose kernel keeps its "
                                       "work area in global memory (pass an explicit stream)");
    hipError_t e = clik::qp_launch_data(h->variant, h->dev, h->warm, tk, (long long)B, h->host.d.n_y, q, x, y, Hdiag, A,
                                        lbA, ubA, (hipStream_t)stream, h->gws.get());
    if (e != hipSuccess) return hipfail(e, "qp_data_kernel launch");
    return CLIK_OK;
}
