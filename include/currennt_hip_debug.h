/*
 * currennt_hip_debug.h -- kernel-level test hooks of libcurrennt_hip.so.
 *
 * Not part of the drop-in boundary: these run one GEMM kernel on host-provided fp32 matrices (converted to
 * the context's operand type on the device) so the tests can check the MFMA kernels in isolation against
 * the oracle's helpers::Matrix restatement (helpers/Matrix.cu:41-183).
 */
#ifndef CURRENNT_HIP_DEBUG_H
#define CURRENNT_HIP_DEBUG_H

#include "currennt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C[M][N] = act(A[M][K] * B[N][K]^T + bias[N]);  K % 8 == 0, N % 32 == 0;  act: 0 tanh, 1 logistic, 2 identity;
 * act | 0x100: the kernel writes the fp32 result AND its operand-type copy (what a hidden feed-forward layer asks for) and the
 * copy is returned (widened to float); act | 0x200: the copy alone */
int cn_dbg_gemm_nt(cn_ctx *ctx, const float *A, const float *B, float *C, int M, int N, int K,
                   const float *bias, int act);
/* C[M][N] = A[K][M]^T * B[K][N];  M % 32 == 0, N % 32 == 0 */
int cn_dbg_gemm_tn(cn_ctx *ctx, const float *A, const float *B, float *C, int M, int N, int K);
/* The weight-gradient products as a layer launches them (launch_gemm_tn_group: the three products of an LSTM layer, a dense
 * layer's one): up to three products side by side, each on VIEWS into host-provided fp32 parents.
 *   A parent [rows_a][lda], view rows a_row .. a_row + K - 1, columns a_col .. a_col + M - 1
 *   B parent [rows_b][ldb], view rows b_row .. b_row + K - 1, columns b_col .. b_col + N - 1
 *   C [M][ldc], ldc >= N, uploaded AS GIVEN (pre-zeroed where the sums go; the pitch columns may hold sentinels) and returned
 * The parents are converted to the context's operand type whole (items that name the same host parent share one device copy),
 * the views are pointer arithmetic on the copies.  An item with M, N or K == 0 is skipped.  M, N multiples of 32; every view
 * inside its parent; pitches and column offsets multiples of 16 bytes in the operand type (4 floats, 8 bf16). */
typedef struct cn_dbg_tn_item {
    const float *A; int rows_a, lda;
    const float *B; int rows_b, ldb;
    int a_row, a_col, b_row, b_col;
    int M, N, K;
    float *C; int ldc;
} cn_dbg_tn_item;
/* dst[r][c] (+)= part[0][r][c] + part[1][r][c] + ... in that order, r < rows, c < cols <= ld; host dst [rows][ld], host part
 * [nparts][stride] (partials share dst's pitch, stride >= (rows - 1) * ld + cols); clear: the partials read are zeroed. */
typedef struct cn_dbg_fold_item {
    float *dst; float *part; long long stride;
    int nparts, rows, cols, ld, accumulate, clear;
} cn_dbg_fold_item;
/* what the hook fills a deterministic product's workspace with before the launch */
#define CN_DBG_WS_SENTINEL (-1234.5f)
#define CN_DBG_MAX_SPLITS 8
/* n <= 3 items, cu_budget as launch_gemm_tn_group's (0 = the chip).  Context option "deterministic" on: every item gets a
 * workspace of CN_DBG_MAX_SPLITS * M * ldc floats filled with CN_DBG_WS_SENTINEL.
 * flags & 1 (deterministic contexts only): the deferred form -- no fold is launched, splits_out[i] (required) = the splits
 * item i was cut into (0: skipped), and item i's C is [CN_DBG_MAX_SPLITS][M][ldc]: the whole workspace comes back, nothing is
 * uploaded from it.
 * extra (nullable): one more fold that rides on the call's last launch; its dst is returned, and its part when clear is set.
 * Everything is validated before anything is launched (CN_ERR_SHAPE / CN_ERR_BAD_ARG).  [sync] */
int cn_dbg_gemm_tn_group(cn_ctx *ctx, const cn_dbg_tn_item *items, int n, int cu_budget, int flags, int *splits_out,
                         const cn_dbg_fold_item *extra);
/* launch_fold on host-provided partials; n may exceed the items of one launch.  Every dst is returned, and every part whose
 * item has clear set.  [sync] */
int cn_dbg_fold(cn_ctx *ctx, const cn_dbg_fold_item *items, int n);
/* The row map of the fraction that is loaded (no counterpart in the reference, which multiplies every frame of a fraction:
 * LstmLayer.cu:771-786): out[0] frames whose rows the N-wide products compute, out[1] dummy frames whose rows they fill with
 * bias / 0 instead, out[2] T x (padded) parallel sequences.  [sync] */
int cn_dbg_row_map_counts(cn_ctx *ctx, int out[3]);
/* Loads of this context that found their fraction announced and re-laid out (cn_fraction_prefetch / _resident) and only exchanged
 * buffers. */
int cn_dbg_prefetch_hits(cn_ctx *ctx, int *hits);
/* The time axis a layer runs on (include/currennt_hip.h, section Strided context layers), as the device holds it for the current
 * fraction: pat [T' * PSp] pattern types and tcls [T' * PSp] classes in the DEVICE's row order (row j * PSp + s, pad slots
 * included), len [PSp] slot lengths; any pointer may be NULL.  rows must be T' * PSp (CN_ERR_SHAPE); an axis that has not been
 * formed for the current fraction: CN_ERR_STATE.  [sync] */
int cn_dbg_layer_axis(cn_layer *layer, char *pat, int *tcls, int *len, size_t rows, int *PSp);
/* What a read-back in the reference layout cannot show: the number of elements with a non-zero bit in the pad columns and pad
 * slots of the operand rows the layer's followers read (T' * PSp rows of the padded pitch, the current fraction).  [sync] */
int cn_dbg_layer_pad_bits(cn_layer *layer, long long *nonzero);

/* The launches of a CN_LAYER_CTC layer (csrc/cn_ctc.hip: the sweeps, then the output errors) on posteriors of the caller's choice.
 * Host arrays in the reference layout: y [T * PS][C] posteriors (blank = C - 1), pat [T * PS] pattern types, the labels as for
 * cn_layer_set_label_sequences with one length per slot (PS of them); out: loss_out [PS] = -log p per slot (0 for a sequence
 * without an alignment), err_out [T * PS][C] = dL/dy.  The device buffer of the output errors starts as NaNs, and the hook fails
 * with CN_ERR_STATE when a pad slot or pad column of it is not exactly 0.  [sync] */
int cn_dbg_ctc(cn_ctx *ctx, const float *y, const char *pat, int T, int PS, int C, const int *labels, const int *label_lengths,
               float *loss_out, float *err_out);
/* The launches of CTC decoding (include/currennt_hip.h, section CTC decoding; csrc/cn_ctc_decode.hip) on posteriors of the caller's
 * choice.  Host arrays as for cn_dbg_ctc; label_lengths == NULL: a fraction without labels (every distance is -1).  The pad
 * columns of the device's rows hold +inf: they would win every row if they took part.  accumulate != 0: the context's sums take
 * the fraction's numbers (cn_ctc_decode_read), which needs labels (CN_ERR_STATE).  out, any may be NULL: argmax_out [T * PS] the
 * index per frame (-1 for a frame with pattern type 0), decoded [PS][T], decoded_lengths [PS], distances [PS].  The hook fails
 * with CN_ERR_STATE when a pad slot decodes to anything.  [sync] */
int cn_dbg_ctc_decode(cn_ctx *ctx, const float *y, const char *pat, int T, int PS, int C, const int *labels, const int *label_lengths,
                      int accumulate, int *argmax_out, int *decoded, int *decoded_lengths, int *distances);

/* The masked operand copy a dropping layer's input products read (include/currennt_hip.h, section Dropout), as its last forward
 * pass left it: reference layout [T * PS][P], P the preceding layer's size, widened to float; count = T * PS * P.  CN_ERR_STATE
 * when that pass did not drop.  [sync] */
int cn_dbg_dropout_input(cn_layer *layer, float *host, size_t count);

/* The weights a layer's last backward pass read (include/currennt_hip.h, section Weight noise): gathered back from the noisy
 * operand copies into the flat reference layout and widened to float; count = cn_layer_weight_count.  Bias entries, which no
 * backward pass reads, are the clean weights.  CN_ERR_STATE when that pass had no noise, and when any pad entry of a noisy copy is
 * not exactly 0.  [sync] */
int cn_dbg_noisy_weights(cn_layer *layer, float *host, size_t count);

/* The branch output of a residual layer (include/currennt_hip.h, section Residual connections), as its last forward pass left it:
 * the layer's own operand copy in the reference layout [T * PS][size], widened to float; count = T * PS * size.  CN_ERR_STATE when
 * that pass did not sum.  [sync] */
int cn_dbg_residual_branch(cn_layer *layer, float *host, size_t count);

/* The normalised copy of a layer's input (include/currennt_hip.h, section Layer normalization), as its last forward pass left it:
 * reference layout [T * PS][P], P the preceding layer's size, widened to float; count = T * PS * P, anything else: CN_ERR_SHAPE.
 * CN_ERR_STATE when that pass did not normalise.  A layer that also drops keeps both copies: cn_dbg_dropout_input returns what
 * its input products read, the masked copy of this one.  [sync] */
int cn_dbg_layer_norm_input(cn_layer *layer, float *host, size_t count);

#ifdef __cplusplus
}
#endif
#endif
