// Fold-in (als_fold_in): the factor row of a query that was not in the training block, from its ratings and the
// resident opposite factors -- x = (Y_S^T Y_S + lambda n I)^-1 Y_S^T r, the reference's normal equation
// (MFeatureCalculator.java:85-99), over ad-hoc rows. A serving path: one to a few thousand short rows per call, no work
// plan, no padded in-block, no per-engine state.
//
// The kernel is als_fold_solve_kernel<T, KP, FoldinArgs> of als_fold_solve.h, which describes it: one 256-thread
// workgroup owns one whole query, the Gram Y^T Y on the matrix pipe at full input precision, the right-hand side Y^T r
// on the VALU, lambda n on the diagonal, a register Cholesky, and in fp64 one refinement step with the residual
// sum_e y_e (r_e - y_e . x) - lambda n x.
// DESIGN.md section 3.9 has the layout, the resource figures and the measurements.
#include <climits>
#include <type_traits>

#include "als_device.h"

namespace cfk {
namespace {

#include "als_fold_tiles.h"   // accumulator types, tile maps, fold_gram_batch, fold_store_tiles, FoldBatch
#include "als_fold_solve.h"   // als_fold_solve_kernel, fold_by_kp, fold_plan_ok, launch_fold_solve

}  // namespace

hipError_t launch_fold_in(int precision, int kp, const FoldinArgs& a, const FoldinPlan& plan, hipStream_t s) {
    if (a.n_queries <= 0) return hipSuccess;
    if (!fold_plan_ok(precision, kp, a, plan)) return hipErrorInvalidValue;
    return precision == 0 ? launch_fold_solve<float>(kp, a, plan, s) : launch_fold_solve<double>(kp, a, plan, s);
}

}  // namespace cfk
