// The draw tile: what the per-row kernels that walk the uploaded rows against every posterior draw share (textually
// included by fokl_hip.hip ahead of them) -- predict_mfma_kernel, score_kernel, predictive_kernel and, for the tile load
// only, design_quadform_kernel.  One wavefront per tile of 16 rows; lane l has col = l & 15 (its row of the tile) and
// quad = l >> 4 (its quarter of the draws).  The host side of the format is fill_draw_table (fokl_hip.hip).
//
// All four call draw_tile_load.  draw_product is called by predictive_kernel; predict_mfma_kernel and score_kernel hold
// the same text written out in their draw loops, because the compiler arranges the k loop of the inlined function otherwise
// (the accumulators leave the matrix pipe's registers in an exit block of their own, about 30 instructions more) and that
// form measured 1 to 3 % slower in both (docs/LAB_NOTEBOOK.md, "The draw tile").  Whoever changes the format below changes
// it in draw_product and in those two loops; a new kernel calls draw_product.

namespace fokl {

// The tile's basis values into LDS: xs[k * 16 + col] = column slots[k] of row r for k < nc, 0.0 for the padding columns
// nc <= k < kp and for rows past n (`in` false), so that neither ever contributes to a product.  kp is the k extent of the
// product that follows (the columns rounded up to 4, or to 16 for the design's matrices).  The caller's __syncthreads()
// orders the stores against the product's reads.
__device__ __forceinline__ void draw_tile_load(double *xs, double *const *__restrict__ slot_ptr, const int *__restrict__ slots,
                                               int nc, int kp, int64_t r, bool in, int quad, int col)
{
    for (int k = quad; k < kp; k += 4)
        xs[k * 16 + col] = (in && k < nc) ? *(__attribute__((address_space(1))) const double *)(slot_ptr[slots[k]] + r) : 0.0;
}

// The rows-by-draws product of one block of DT x 16 draws: acc[t][v] = X_row . beta_d for row col and draw
// d = d0 + 16 t + quad + 4 v.
//   * betas_t is the coefficient table transposed and zero padded on the host to [ncp][dp], ncp = columns rounded up to 4,
//     dp = draws rounded up to 16: the A fragment of one k-step is one 128-byte run per term, and padding columns and
//     draws multiply zeros.
//   * D[draw][row] comes out of v_mfma_f64_16x16x4_f64 (A = 16 draws x 4 terms, B = 4 terms x 16 rows out of xs): lane l
//     supplies A[draw = col][term = quad] and B[term = quad][row = col] and ends up with D[quad + 4 v][col], v = 0 .. 3,
//     i.e. with a quarter of the block's draws of ONE row.  The DT tiles are independent chains for the matrix pipe.
//   * A 16-draw tile past dp (d0 + 16 t >= dp, in the last block only) re-reads the last tile of the table instead of
//     running off its end; its accumulators hold that tile's values and the caller skips them, as it skips the padding
//     draws d >= draws.
//   * The coefficients of the next k-step are loaded in front of this step's MFMAs, so that they travel while the pipe
//     works; the last step re-reads its own.
template <int DT>
__device__ __forceinline__ void draw_product(const double *xs, const double *__restrict__ betas_t, int ncp, int dp, int d0,
                                             int quad, int col, d4 (&acc)[DT])
{
    const double *a_ptr[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) {
        acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
        a_ptr[t] = betas_t + (size_t)quad * dp + min(d0 + 16 * t, dp - 16) + col;
    }
    double a_now[DT], a_next[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) a_now[t] = a_ptr[t][0];
    for (int k0 = 0; k0 < ncp; k0 += 4) {
        const double b = xs[(k0 + quad) * 16 + col];
        const int kn = k0 + 4 < ncp ? k0 + 4 : k0;
#pragma unroll
        for (int t = 0; t < DT; ++t) a_next[t] = a_ptr[t][(size_t)kn * dp];
#pragma unroll
        for (int t = 0; t < DT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a_now[t], b, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < DT; ++t) a_now[t] = a_next[t];
    }
}

}  // namespace fokl
