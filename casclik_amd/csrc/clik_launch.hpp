// What clik_api.hip calls in the translation units that hold the kernels: kernel tables, their selectors and launchers.
// The units that define these functions include this header as well, so that the compiler holds every definition
// against its declaration.  Host declarations only - no kernel header includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "clik_device.hpp"

namespace clik {
struct LaunchArgs;      // clik_pinv_select.hpp
struct GwsOwner;        // clik_workspace.hpp

// ---- clik_pinv.hip: the pseudo-inverse kernels (ahead-of-time shapes and the dynamic widths) ---------------------------
int pinv_pick_kernel(const DevSkill& S, int allow_static);
const char* pinv_kernel_name(int k);
int pinv_kernel_width(int k);
int pinv_kernel_is_static(int k);
hipError_t pinv_launch_solve(int k, const LaunchArgs& a, const TickArgs& tk, long long B, const double* q,
                             const double* x, const double* y, double* dq, double* dx, int32_t* mode,
                             hipStream_t stream);
hipError_t pinv_launch_rollout(int k, const LaunchArgs& a, const double* d_tterms, int n_ticks, double dt,
                               double max_speed, long long B, double* q, const double* y, double* dq,
                               int32_t* mode, hipStream_t stream);
int pinv_lds_slots_host(int N, int ny);
// resident ticks: waves per tick of the four-lanes-per-instance launch, and the reference producer
int team_waves_rt(long long B);
hipError_t launch_ticket_feed(void* ticket, const unsigned* done, int n_ticks, int closed_loop, unsigned waves_per_tick,
                              unsigned long long timeout_ticks, hipStream_t stream);

// ---- clik_qp.hip: the dynamic-shape QP kernels ---------------------------------------------------------------------------
int qp_pick_variant(int n, int nv, int nc);
int qp_variant_width(int k);
size_t qp_variant_lds(int k, int ny);
bool qp_variant_uses_workspace(int k);
hipError_t qp_launch_solve(int k, const DevSkill* dS, const WarmArgs& wa, const TickArgs& tk, long long B, int ny,
                           const double* q, const double* x, const double* y, double* dq, double* dx,
                           double* slack, int32_t* status, hipStream_t stream, GwsOwner* owner);
hipError_t qp_launch_data(int k, const DevSkill* dS, const WarmArgs& wa, const TickArgs& tk, long long B, int ny,
                          const double* q, const double* x, const double* y, double* Hd, double* A, double* lb,
                          double* ub, hipStream_t stream, GwsOwner* owner);

// ---- clik_qp_shapes.hip: the ahead-of-time shape-specialised QP kernels --------------------------------------------------
int qp_pick_static(const ShapeDesc& sd);
const char* qp_static_name(int k);
hipError_t qp_launch_static(int k, const void* d_img, const TickArgs& tk, long long B, const double* q,
                            const double* x, const double* y, double* dq, double* dx, double* slack,
                            int32_t* status, int32_t* hot_set, int use_hot, hipStream_t stream,
                            const double* t_inst);
hipError_t qp_launch_rollout_static(int k, const void* d_img, const double* d_tterms, int n_ticks, double dt,
                                    double max_speed, long long B, double* q, const double* y, double* dq,
                                    double* slack, int32_t* status, double* x, double* dx, hipStream_t stream,
                                    int stages);
}  // namespace clik
