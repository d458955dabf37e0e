// ===========================================================================
// route.hpp -- the routing seam between the dispatcher (abi.hip) and the organisations it chooses from: the answer type
// of the functions that may decline a call, and the one declaration of every function that crosses a translation unit here.
//
// Two families, two types:
//   * ROUTES (`Route`): try_*, routed_*, owner_pull_prepare, launch_push_bricks and the file-local launchers whose answer they pass on.
//     "Did this organisation take the call?" -- declined (nothing launched that the caller's fallback would not overwrite), done,
//     gated (enqueued behind a probe's gate: the caller enqueues the other organisations behind the same gate), or failed with a code.
//   * STATUSES (`int`): launch_*_<dtype>, the probes, owner_pull_finish, mix_launch_*, big_lds, the Defer members.  0 is ok, anything
//     else an error: a negative INTERPOL_E_* or a positive hipError_t.
// hipErrorInvalidValue is 1 and hipErrorOutOfMemory is 2, so a status must never be read as a route.  Route converts to and from
// nothing; a status enters one only through Route::error (IP_TRY, Route::done_unless), and leaves through abi_code().
// ===========================================================================
#pragma once
#include "../../include/interpol_hip.h"
#include "stencil.hpp"
#include "filter_params.hpp"
#include "defer.hpp"
#include <hip/hip_runtime.h>

namespace ip {

class [[nodiscard]] Route {
public:
    static constexpr Route declined() { return Route(DECLINED, 0); }
    static constexpr Route done() { return Route(DONE, 0); }
    static constexpr Route gated() { return Route(GATED, 0); }
    static constexpr Route error(int code) { return Route(FAILED, code ? code : (int)INTERPOL_E_LAUNCH); }   // code: INTERPOL_E_* or (int)hipError_t
    static constexpr Route done_unless(int status) { return status ? error(status) : done(); }               // the last launch of an organisation
    constexpr bool failed() const { return took_ == FAILED; }
    constexpr bool is_declined() const { return took_ == DECLINED; }
    constexpr bool is_done() const { return took_ == DONE; }
    constexpr bool is_gated() const { return took_ == GATED; }
    constexpr int abi_code() const { return code_; }             // 0 unless failed(): what an interpol_* entry point returns
private:
    enum Took { DECLINED, DONE, GATED, FAILED };
    constexpr Route(Took t, int c) : took_(t), code_(c) {}
    Took took_;
    int code_;
};

static_assert(Route::error((int)hipErrorInvalidValue).failed() && !Route::error((int)hipErrorInvalidValue).is_done()
              && Route::error((int)hipErrorInvalidValue).abi_code() == 1, "HIP error 1 is an error, not `done`");
static_assert(Route::error((int)hipErrorOutOfMemory).failed() && !Route::error((int)hipErrorOutOfMemory).is_gated()
              && Route::error((int)hipErrorOutOfMemory).abi_code() == 2, "HIP error 2 is an error, not `gated`");
static_assert(Route::done().abi_code() == 0 && Route::gated().abi_code() == 0 && Route::declined().abi_code() == 0
              && !Route::done().failed() && !Route::gated().failed() && !Route::declined().failed(), "a route is not an error");

// a status inside a function that answers with a Route: go on when it is 0, else leave with the error
#define IP_TRY(status) do { const int s_ = (status); if (s_) return ::ip::Route::error(s_); } while (0)

// ---- statuses: the generic kernels (ops_instantiate.inc, affine_grad.hip) and the single-organisation operators --------------------
#define IP_DECL(sfx)                                                                                                   \
    int launch_pull_##sfx(const KParams &, const void *, const void *, void *, int, hipStream_t);                     \
    int launch_grad_##sfx(const KParams &, const void *, const void *, void *, int, hipStream_t);                     \
    int launch_push_##sfx(const KParams &, const void *, const void *, void *, int, hipStream_t);                     \
    int launch_pullbwd_##sfx(const KParams &, const void *, const void *, const void *, void *, void *, int, int64_t, int64_t, hipStream_t); \
    int launch_pushbwd_##sfx(const KParams &, const void *, const void *, const void *, void *, void *, int, hipStream_t); \
    int launch_narrow_##sfx(const void *, void *, int64_t, hipStream_t);                                               \
    int launch_affine_grad_##sfx(const KParams &, const void *, const void *, const void *, void *, void *, int, hipStream_t);
IP_DECL(f32) IP_DECL(f64) IP_DECL(bf16) IP_DECL(f16)
#undef IP_DECL
#define IP_DECL2(sfx)                                                                                                  \
    int launch_hess_##sfx(const KParams &, const void *, const void *, void *, int, hipStream_t);                     \
    int launch_pushgrad_##sfx(const KParams &, const void *, const void *, void *, int, hipStream_t);
IP_DECL2(f32) IP_DECL2(f64)
#undef IP_DECL2

int launch_filter(int dtype, const FilterParams &fp, const void *src, void *data, hipStream_t st);
bool resample1d_adjoint_gathers(int64_t n_samples, int64_t inner);
int launch_resample1d(int dtype, int lin_f64, int order, const KParams &p, int adjoint, const void *src, const void *lin, void *dst,
                      unsigned ns, unsigned inner, int64_t nl, int64_t outer, hipStream_t st);
int launch_pull_labels(const KParams &p, int grid_f64, const void *vol, const void *grid, void *val, int B, hipStream_t st);

// ---- routes: the LDS tiles, one translation unit per storage type ------------------------------------------------------------------
// try_fast_* (ops_tiled.hip) ask the organisations below in turn and end at the natural-order tiles
#define IP_DECL_TILED(sfx)                                                                                             \
    Route try_fast_pull_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route try_fast_grad_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route try_fast_push_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route try_fast_pullbwd_##sfx(const interpol_problem *, const KParams &, const void *, const void *, const void *,   \
                                 void *, void *, int64_t, int64_t, hipStream_t);                                       \
    Route try_fast_pushbwd_##sfx(const interpol_problem *, const KParams &, const void *, const void *, const void *,   \
                                 void *, void *, hipStream_t);                                                         \
    /* class-sorted tiles (ops_sorted.hip): 3-D, one order 1..3, or mixed orders 1..3 (a module of their own) */       \
    Route try_sorted_pull_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route try_sorted_gradc_##sfx(const interpol_problem *, const KParams &, const void *, const void *, const void *, void *, hipStream_t); \
    Route try_sorted_push_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route sorted_pull_mixed_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route sorted_gradc_mixed_##sfx(const interpol_problem *, const KParams &, const void *, const void *, const void *, void *, hipStream_t); \
    /* lean 2-D tiles (ops_tiled2d.hip): per-dim orders 1..3 */                                                        \
    Route try_tiled2d_pull_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    Route try_tiled2d_gradc_##sfx(const interpol_problem *, const KParams &, const void *, const void *, const void *, void *, hipStream_t); \
    Route try_tiled2d_push_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    /* 1-D scatter tiles (push1d.hip) */                                                                               \
    Route try_push1d_##sfx(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t); \
    /* (experiments/pull_window.hip) the windowed gather: every sample visited once -- measured slower, not in the product */ \
    Route try_window_pull_##sfx(const interpol_problem *, const KParams &, int, const void *, const void *, void *, hipStream_t);
IP_DECL_TILED(f32) IP_DECL_TILED(bf16) IP_DECL_TILED(f16)
#undef IP_DECL_TILED
// (experiments/pull_direct.hip)
Route try_pull_direct(const interpol_problem *, const KParams &, const void *, const void *, void *, int *, int, hipStream_t);

// float64 scatter on LDS tiles (push_f64.hip)
Route try_push_f64_tiles(const interpol_problem *, const KParams &, const void *, const void *, void *, hipStream_t);

// ---- the bricks: owner-computes scatter and its gathers for same-resolution deformations (push_owner.hip) --------------------------
int64_t owner_workspace_bytes(const interpol_problem *, const KParams &, bool);
Route try_owner_push(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, hipStream_t, const int **, PendingZero *);
int64_t owner_pull_workspace_bytes(const interpol_problem *, const KParams &);
Route owner_pull_prepare(const interpol_problem *, const KParams &, void *, int64_t, hipStream_t, int **, int *);      // declined / done
int owner_pull_finish(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, bool, hipStream_t,
                      bool grad = false, const void *gout = nullptr, bool probed = false, bool spatial = false);
int owner_grad_probe(const interpol_problem *, const KParams &, const void *, void *, int64_t, hipStream_t, int mode = -1);
int linear_pull_probe(const interpol_problem *, const KParams &, const void *, void *, hipStream_t, const int **, int);
// orders 4 - 5 (gather5.hip) and 6 - 7 (gather7.hip: the same file, its own module); the 5s hand orders >= 6 to the 7s
#define IP_DECL_G5(n)                                                                                                   \
    int64_t gather##n##_workspace_bytes(const interpol_problem *, const KParams &);                                     \
    int64_t scatter##n##_workspace_bytes(const interpol_problem *, const KParams &);                                    \
    Route try_gather##n(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, int, const void *, hipStream_t, const int **); \
    Route try_scatter##n(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, hipStream_t, const int **); \
    Route try_backward##n(const interpol_problem *, const KParams &, const KParams &, const void *, const void *, const void *, void *, void *, void *, int64_t, \
                          hipStream_t, const int **);                                                                   \
    Route try_pushbwd##n(const interpol_problem *, const KParams &, const void *, const void *, const void *, void *, void *, void *, int64_t, hipStream_t);
IP_DECL_G5(5) IP_DECL_G5(7)
#undef IP_DECL_G5
// 2-D (scatter2d.hip)
int64_t scatter2d_workspace_bytes(const interpol_problem *, const KParams &);
int64_t gather2d_workspace_bytes(const interpol_problem *, const KParams &);
Route try_gather2d(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, int, const void *, hipStream_t, const int **);
Route try_scatter2d(const interpol_problem *, const KParams &, const void *, const void *, void *, void *, int64_t, hipStream_t, const int **);
// the first bricks (push_bricks.hip: interpol_push_bricks); declined: the problem does not fit them
int64_t bricks_workspace_bytes(const KParams &p, int B, int shared);
Route launch_push_bricks(const KParams &p, int B, int shared, const void *val, const void *grid, void *vol,
                         void *workspace, int64_t workspace_bytes, hipStream_t st);

} // namespace ip
