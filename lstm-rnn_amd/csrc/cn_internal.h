// Internal declarations shared by the translation units of libcurrennt_hip.so.
// Nothing in here is part of the ABI (include/currennt_hip.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>

#include "../../include/currennt_hip.h"
#include "cn_unit_map.h"

namespace cn {

// ---- activation ids used by kernels --------------------------------------------------------
enum Act { ACT_TANH = 0, ACT_LOGISTIC = 1, ACT_IDENTITY = 2 };

// kernel classes for cn_ctx_timing_*
enum KClass { KC_REC_FWD = 0, KC_REC_BWD = 1, KC_GEMM_WIDE = 2, KC_GEMM_GRAD = 3, KC_OTHER = 4, KC_COMM = 5, KC_COUNT = 6 };

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Arithmetic of the MFMA products (`prec` arguments of the launchers below).  The values of P_BF16 / P_F32 equal
// false / true, so a caller that only knows "fp32 operands or not" may pass a bool.
//   P_BF16  bf16 operands in memory and in the MFMAs (throughput mode)
//   P_F32   fp32 operands in memory, exact-fp32 MFMAs (v_mfma_f32_*_f32, 1/16 of the bf16 rate)
//   P_X3    fp32 operands in memory; every operand is split in the kernel into bf16 hi + bf16 lo (x = hi + lo + O(2^-17 x))
//           and a product is three bf16 MFMAs (hi*hi + lo*hi + hi*lo, fp32 accumulation): ~2^-16 relative per term, a third
//           of the bf16 rate -- the parity mode that is fast (CN_PREC_BF16X3)
enum Prec { P_BF16 = 0, P_F32 = 1, P_X3 = 2 };

// ---- options -----------------------------------------------------------------------------------
// ONE block of A/B and test switches per context instead of environment look-ups scattered over the launch paths (round 6).  A context
// copies the process defaults -- read ONCE from the environment, variable CN_<NAME IN CAPITALS> -- at cn_ctx_create; after that
// only cn_ctx_set_option(ctx, "<name>", value) changes them, and no launch path reads the environment.  FLAG: set by the mere
// presence of the variable (as before); NUM: its integer value.  Options that size allocations (cluster4, no_cluster, rpl) must be
// set before the layers are created.  cn_layer_recurrent_kernel keeps reporting which kernel actually ran.
#define CN_OPTION_LIST(FLAG, NUM)                                                                                                  \
    /* GEMM selection */                                                                                                          \
    FLAG(no_big_gemm) FLAG(no_big8) NUM(big8_min_k, 0) FLAG(no_nt_mid) FLAG(no_big_tn) NUM(nt_bm64_below, 400) NUM(tn_blocks, 0) \
    NUM(tnbig_blocks, 0) NUM(tnbig_group_mink, 28000) NUM(nt_mid_min_tiles, 384) NUM(nt_bm64_shortk_tiles, 1100) FLAG(no_nt_panel) NUM(nt_panel_max_panels, 0) FLAG(nt_panel_no_touch) NUM(nt_panel_min_ktiles, 8) NUM(nt_panel_max_ntiles, 2) FLAG(no_nt_rowmap) FLAG(nt_rowmap_tiled)                                                                           \
    /* recurrent kernel selection */                                                                                              \
    FLAG(no_lds_claim) FLAG(bwd_ug2) FLAG(fwd_ug2) FLAG(bwd_psum) FLAG(no_bwd_psum) FLAG(cluster_helpers) FLAG(no_cluster_helpers) \
    FLAG(cluster4) FLAG(no_cluster) FLAG(cluster_gate_off) FLAG(no_s2c) FLAG(s2c) FLAG(no_s2_asm) FLAG(no_s2_asm_bwd) FLAG(s2_x3) \
    FLAG(no_s2) FLAG(no_s2w) FLAG(no_s2w_asm) FLAG(pre16)                                                                           \
    /* step structure */                                                                                                          \
    FLAG(softmax_exact) FLAG(tail_on_side) FLAG(no_side_rule) FLAG(no_lazy_softmax) FLAG(lazy_softmax) FLAG(comm_test_double)     \
    FLAG(no_loss_defer) FLAG(no_pack_group) FLAG(no_sgd_fuse) NUM(comm_cu_margin, 32)                                           \
    /* CTC: label cap per sequence of a CTC layer created afterwards (0: min(max_seq_length, 512)); A/B: the beta sweep as a     \
       launch of its own behind the alpha sweep instead of beside it */                                                          \
    NUM(ctc_max_labels, 0) FLAG(ctc_serial_sweeps)                                                                                \
    /* CTC decoding, measurement only (tools/ctc_decode_cost.py): the argmax launch alone, nothing is collapsed or counted */    \
    FLAG(ctc_decode_argmax_only)                                                                                                  \
    /* weight noise: generate the noisy operand copies on the side stream beside the forward pass (the key is known before it) \
       instead of on the main stream in front of the first backward kernel */                                                    \
    FLAG(noise_ahead)
struct Options {
#define CN_OPT_FIELD(name) int name = 0;
#define CN_OPT_FIELD_NUM(name, dflt) long name = dflt;
    CN_OPTION_LIST(CN_OPT_FIELD, CN_OPT_FIELD_NUM)
#undef CN_OPT_FIELD
#undef CN_OPT_FIELD_NUM
};
Options options_from_env();                              // (the environment is read here and nowhere else on the compute path)
bool option_set(Options &o, const char *name, long value);  // false: no such option
bool option_get(const Options &o, const char *name, long *value);
// the options of the context whose call is running on this thread (set by every entry point of the ABI that touches the
// device); the process defaults outside of one
const Options &opt();

// hipFuncSetAttribute (the > 64 KB dynamic LDS opt-in) is per device: a process may drive several GPUs
struct DeviceOnce {
    std::atomic<unsigned long long> seen{0};
    bool first()
    {
        int d = 0;
        (void)hipGetDevice(&d);
        const unsigned long long bit = 1ull << (d & 63);
        return (seen.fetch_or(bit) & bit) == 0;        // (contexts of several host threads may launch concurrently)
    }
};

// ---- GEMM ------------------------------------------------------------------------------------
// All matrices are row-major; "op" element type is float (CN_PREC_F32) or bf16 (CN_PREC_BF16).
struct GemmNT {            // C[m][n] = sum_k A[m][k] * B[n][k]   (+ bias[n]) -> act -> C / C2
    const void *A; long lda;      // [M][K] op
    const void *B; long ldb;      // [N][K] op
    float *C; long ldc;           // [M][N] fp32 (nullable)
    void *C2; long ldc2;          // [M][N] op copy (nullable)
    const float *bias;            // [N] fp32 added before the activation (nullable)
    int act;                      // Act
    int M, N, K;                  // K multiple of 8 (bf16) / 4 (f32); N multiple of 32
    // Row map of the fraction (launch_rowmap; nullable): rowcnt[0] real frames whose rows are rowmap[0 ..), rowcnt[1] dummy ones
    // (patType NONE at a time step where the kernels check it: pad slots, frames behind the end of a sequence) in dummymap[0 ..).  A kernel that takes the map computes the
    // real rows only and writes bias[n] (or 0) into the dummy rows -- what the full product gives there, because every operand row
    // of a dummy frame is zero (zero-padded inputs, y = 0 by ComputeBlockOutputFn's dummy rule, deltas = 0 by ComputeBlockErrorsFn's).
    // Kernels that do not take it compute all M rows.  m_est: the host's estimate of rowcnt[0] (0: M), for the dispatch only.
    const int *rowmap, *dummymap, *rowcnt; int m_est;
};
struct GemmTN {            // C[m][n] += sum_k A[k][m] * B[k][n]   k in [0,K), fp32 atomics (split-K)
    const void *A; long lda;      // [K][M] op
    const void *B; long ldb;      // [K][N] op
    float *C; long ldc;           // [M][N] fp32, pre-zeroed
    int M, N, K;                  // M, N multiples of 32
    // deterministic mode (cn_ctx option "deterministic"): split s STORES its partial product to ws + s * M * ldc (same pitch as
    // C) and a second launch adds the partials IN SPLIT ORDER into C -- the sum over the frames no longer depends on the order in
    // which workgroups retire (ComputeWeightUpdateFn, LstmLayer.cu:289-512, is one serial sum per weight).  nullptr: fp32 atomics.
    float *ws; int ws_splits;     // workspace of ws_splits * M * ldc floats; the launcher never cuts K into more splits than that
    // ws_used (host pointer, nullable): the launcher writes the number of splits it cut there and does NOT launch the fold -- the
    // caller's consumer adds the partials itself (pack_group_kernel in its update = 2 form: no extra launch behind the product)
    int *ws_used;
};
constexpr int DET_MAX_SPLITS = 8;
// dst[r][c] (+)= part[0][r][c] + part[1][r][c] + ... in that order, r < rows, c < cols (partials share dst's pitch `ld`, one every
// `stride` floats).  accumulate: onto what dst holds (else dst is overwritten); clear: the partials are zeroed behind the read.
struct FoldItem { float *dst; float *part; long stride; int nparts, rows, cols, ld, accumulate, clear; };
constexpr int FOLD_MAX = 4;
void launch_fold(hipStream_t s, const FoldItem *items, int n);
// ---- what the GEMM launchers share (cn_gemm.hip) ----
int device_cus();                                        // CUs of the current device (looked up once per device)
// eligibility of the LDS-DMA kernels: rows of `elt`-byte elements, `ld` elements apart from `base`, start on multiples of `align` bytes
bool rows_aligned(const void *base, long ld, int elt, int align);
// ... `rows` such rows end below byte offset `limit` (what a 32-bit buffer offset reaches)
bool rows_fit(long rows, long ld, int elt, unsigned long long limit);
// ... the result rows take whole 16-byte stores of four columns: fp32 C and / or bf16 C2 (a null pointer passes)
bool nt_out_rows_aligned(const GemmNT &g);
// The tail of split-K planning, the same for every gemm_tn launcher: cut K into about `splits` chunks of whole k-tiles (bk frames),
// return the number of chunks that makes (*kchunk frames each), and hand the deterministic mode its count: to *g.ws_used, or as a
// fold of the partials appended to fold[*nfold].  (How many splits to ASK for is each launcher's own policy.)
int tn_plan_splits(const GemmTN &g, int splits, int bk, int *kchunk, FoldItem *fold, int *nfold);
// `done`: optional event that completes with the kernel itself (hipExtLaunchKernelGGL stop event): a fork point for
// another stream without a marker packet on this stream (an hipEventRecord between two kernels costs the second one ~7 us)
void launch_gemm_nt(hipStream_t s, int prec, const GemmNT &g, hipEvent_t done = nullptr);
// 256 x 256 LDS-DMA variant for the MFMA-bound shapes (cn_gemm_big.hip); launch_gemm_nt dispatches to it
bool gemm_nt_big_applies(int prec, const GemmNT &g);
void launch_gemm_nt_big(hipStream_t s, int prec, const GemmNT &g, hipEvent_t done = nullptr);
// 128 x 256 tiles, two workgroups per CU, for the output-bound short-K products (cn_gemm_nt_mid.hip)
bool gemm_nt_mid_applies(int prec, const GemmNT &g);
// one 64-row panel per CU walked as one fill pipeline, for the N-wide products of short fractions (cn_gemm_nt_panel.hip)
bool gemm_nt_panel_applies(int prec, const GemmNT &g, int cus);
void launch_gemm_nt_panel(hipStream_t s, const GemmNT &g, hipEvent_t done = nullptr);
void launch_gemm_nt_mid(hipStream_t s, const GemmNT &g, hipEvent_t done = nullptr);
// cu_budget: CUs the launch may fill with its one-per-CU workgroups when it goes to the 256 x 256 kernel (0 = the chip)
// `extra` (deterministic mode, nullable): one more fold that rides on the launch that adds this product's split partials (the
// layer's bias / peephole / column partial sums): one launch behind the product instead of two
void launch_gemm_tn(hipStream_t s, int prec, const GemmTN &g, int cu_budget = 0, const FoldItem *extra = nullptr);
// 256 x 256 LDS-DMA variant for the products whose operands do not fit the caches (cn_gemm_tn_big.hip); launch_gemm_tn /
// launch_gemm_tn_group dispatch to it
bool gemm_tn_big_applies(int prec, const GemmTN &g);    // on its own
bool gemm_tn_big_can(int prec, const GemmTN &g);        // beside a product that applies (one grouped launch)
void launch_gemm_tn_big_group(hipStream_t s, const GemmTN *gs, int n, int cu_budget = 0, const FoldItem *extra = nullptr);   // n <= 3
void launch_gemm_tn_group(hipStream_t s, int prec, const GemmTN *gs, int n, int cu_budget = 0, const FoldItem *extra = nullptr);      // up to 3 small products in one launch
void launch_gemm_tn_small_group(hipStream_t s, int prec, const GemmTN *gs, int n, const FoldItem *extra = nullptr);   // ... on the 64 x 64 / 128 x 128 tiles whatever their size

// ---- recurrent LSTM kernels --------------------------------------------------------------------
struct LstmRec {
    int H, Hp, dirs, PS, T, Tmin;
    const char *pat;              // [T*PS]
    // forward
    float *acts;                  // [N][dirs][Hp][4] fp32: pre-activations in, n/i/f/o activations out (gate innermost)
    const void *pre16;            // nullable: the pre-activations as bf16 in the same [N][dirs][Hp][4] order (8 bytes per unit and frame);
                                  // the forward kernel then takes them from here and `acts` is output only (lstm_fwd_takes_pre16)
    float *cell;                  // [N][dirs][Hp]    fp32
    float *th;                    // [N][dirs][Hp]    fp32 tanh(cell state), kept by the forward pass for the backward pass
    void  *y_op;                  // [N][dirs*Hp]     op  (layer output, GEMM operand)
    const void *Wrec;             // [dirs][4*Hp][Hp] op  (k = source unit contiguous)
    const float *peep;            // [dirs][3][Hp]
    // backward
    const float *err;             // [N][dirs*Hp] fp32 outputErrors of this layer
    void  *delta_op;              // [N][dirs][Hp][4] op
    const void *WrecT;            // [dirs][Hp][4*Hp] op  (k = 4*target unit + gate contiguous)
    float *dbias;                 // [dirs][Hp][4] fp32 accumulators (pre-zeroed)
    float *dpeep;                 // [dirs][3][Hp]
    float bias;                   // JSON bias value (scales the bias gradient)
    // deterministic mode: workgroup b of the backward kernel STORES its bias / peephole sums into slot b of gpart (a slot: dbias's
    // [dirs][Hp][4] then dpeep's [dirs][3][Hp], 7 * dirs * Hp floats; entries a workgroup does not own stay zero) instead of adding
    // them to dbias / dpeep with atomics; the launcher writes the grid it used to *det_grid (<= gpart_slots or it refuses) and the
    // caller folds the slots in workgroup order (launch_fold, clear = 1).  nullptr: atomics.
    float *gpart; int gpart_slots; int *det_grid;
    int rpl;                      // sequences per lane (1/2/4); PS is a multiple of 4*rpl (padded slots are dummies)
    // multi-CU cluster kernels (cn_lstm_cluster.hip)
    unsigned long long *xch;      // exchange granules (nullable: cluster path off), zeroed at allocation
    unsigned long long *xch_packed;   // ... the packed granules' region of the same buffer (lstm_cluster_xch_packed_offset)
    unsigned xch_epoch;           // tags of this launch are xch_epoch + 1 ... xch_epoch + T (launch_lstm_cluster sets it and advances the counter)
    int *fault;                   // set to 1 by a bounded spin that gave up
    int num_cus;                  // CUs of the device (the one-CU kernels' "does the grid fit the chip in one wave" rule)
    int cluster_cus;              // CUs a cluster grid may count on: a cluster grid must be resident as a whole (spin-wait hand-off),
                                  // so with a communicator bound this is num_cus minus a margin for RCCL's channels
    char *kname;                  // nullable, CN_KNAME_LEN bytes: the launcher writes the name of the kernel it instantiated
};
constexpr int CN_KNAME_LEN = 64;
// every launcher of a recurrent kernel reports its grid (deterministic mode folds that many slots of gpart) and refuses one
// the slots do not cover
void lstm_note_grid(const LstmRec &p, int grid);
// time steps of zeros the library keeps in front of and behind acts / cell / th / err / pat of an LSTM layer (cn_api.cpp:
// dalloc_guarded): a recurrent loop may load up to this many steps outside [0, T)
constexpr int CN_GUARD_STEPS = 6;
size_t lstm_rec_lds_bytes(int prec, bool bwd, int Hp, int rpl, int T);        // dynamic LDS per workgroup of the single-CU kernels
bool lstm_rec_resident(int prec, int Hp);                                      // W_rec fragments register resident (single-CU kernels)
void launch_lstm_forward(hipStream_t s, int prec, const LstmRec &p);
// does the forward kernel launch_lstm_forward would pick for this shape read bf16 pre-activations (LstmRec::pre16)?  The input
// projection then writes 8 instead of 16 bytes per unit and frame -- the N-wide product is bound by that store (round 6).
bool lstm_fwd_takes_pre16(int prec, const LstmRec &p);
// "s2" shape (cn_lstm_s2.hip): two sequences per workgroup, one wave per SIMD, 32 units per wave; launch_lstm_forward /
// launch_lstm_backward dispatch to it when it applies
bool lstm_s2_applies(int prec, const LstmRec &p, bool bwd);
void launch_lstm_s2(hipStream_t s, int prec, bool bwd, const LstmRec &p, hipEvent_t done = nullptr);
bool lstm_s2w_applies(int prec, const LstmRec &p, bool bwd);
void launch_lstm_s2w(hipStream_t s, bool bwd, const LstmRec &p, hipEvent_t done = nullptr);
void launch_lstm_backward(hipStream_t s, int prec, const LstmRec &p, hipEvent_t done = nullptr);   // done: see launch_gemm_nt
// cluster variants for layers whose W_rec exceeds one CU; return false when the shape is not covered
// `num_cus`: the CU count of the device; the spin-wait hand-off needs every member workgroup resident, so a grid larger
// than the device (a partitioned or CU-masked part) does not take the cluster path
size_t lstm_cluster_xch_bytes(int prec, int Hp, int dirs, int PS, int rpl, int num_cus);
size_t lstm_cluster_xch_packed_offset(int prec, int Hp, int dirs, int PS, int rpl, int num_cus);   // bytes from the start of the buffer
int lstm_cluster_size(int prec, int Hp, int dirs, int PS, int rpl, int num_cus);     // CUs per cluster, 0 = path does not apply
// `epoch`: the context's granule-tag counter; the launcher hands tags epoch + 1 ... epoch + T to this launch and advances
// the counter by T + 1, so no caller can forget to (stale granules of an earlier launch never match)
bool launch_lstm_cluster(hipStream_t s, int prec, bool bwd, LstmRec &p, unsigned *epoch);
int lstm_cluster_bwd_cus(int prec, const LstmRec &p);     // CUs the backward cluster launch of this shape occupies (0 = no cluster shape)
void lstm_cluster_stream_gone(hipStream_t s);         // cn_ctx_destroy: the per-device launch gate forgets the stream

// ---- element-wise / packing kernels -----------------------------------------------------------
// (prev, here and in every struct below: the map of the preceding layer's rows, cn_unit_map.h -- its L units are this layer's
// inputs, its Lp columns the pitch of the input operand)
struct LstmGeom { int L, H, Hp, dirs; UnitMap prev; };

// flat fp32 reference weights -> packed op copies + fp32 bias/peephole vectors
void launch_lstm_pack(hipStream_t s, bool f32, const LstmGeom &g, float bias, const float *w,
                      void *Win, void *WinT, void *Wrec, void *WrecT, float *bias_p, float *peep_p);
// packed fp32 gradients -> flat reference layout
// (the packed accumulators are cleared as they are read)
void launch_lstm_unpack_grads(hipStream_t s, const LstmGeom &g, float *dWin, float *dWrec, float *dbias, float *dpeep, float *wu, hipEvent_t done = nullptr);
struct FfGeom { int L, Lp; UnitMap prev; };
// all trainable layers' operand copies in one launch
constexpr int PACK_GROUP_MAX = 8;
// deterministic mode, update == 2: where the partial sums of one packed gradient array lie (nparts == 0: read the packed
// accumulator itself).  The consumer adds part[0], part[stride], ... in that order -- the sum launch_fold would have formed.
struct PackFold { float *part; long stride; int nparts, clear; };
struct PackItem {
    int lstm; LstmGeom lg; FfGeom fg; float bias; const float *w;
    void *Win, *WinT, *Wrec, *WrecT; float *bias_p, *peep_p;
    // update == 1: the momentum-SGD step of SteepestDescentOptimizer.cu:39-59 is applied on the way (every flat weight is read by
    // exactly one packed position, so the thread that packs it also updates it): wd = mom*wd - lr*wu; w += wd
    // Under Adam (a launch with a PackAdam) lr holds the layer's alpha_t, mom holds beta1 and wd is the first moment.
    int update; float *w_rw; const float *wu; float *wd; float lr, mom;
    // update == 2 (cn_ctx_arm_update, no communicator): the gradient is taken straight from the PACKED accumulators the gradient
    // GEMMs / recurrent kernel summed into (every packed position is visited by exactly one thread, which also clears it and
    // writes the flat weightUpdates entry): unpack + update + operand copies in ONE launch behind the layer's gradient GEMMs
    float *wu_rw; float *g_in, *g_rec, *g_bias, *g_peep;      // lstm: dWin, dWrec, dbias, dpeep; ff: dW (g_in), colsum (g_bias)
    // update == 3: ... in deterministic mode from the partial sums their producers stored (PackFold): dWin's splits, dWrec's per direction,
    // the backward workgroups' bias / peephole slots (peephole entries R floats into a slot) or the column-sum rows
    PackFold f_in, f_rec[2], f_bias;
};
struct PackGroup { PackItem item[PACK_GROUP_MAX]; int first[PACK_GROUP_MAX]; int n; };
// The features of an update launch, grouped (launch_pack_group) or flat (launch_flat_update): each is a nullable argument of the
// launcher and a compile-time flag of the one kernel template behind it -- an instantiation holds the code and the kernel
// arguments of the features it was launched with and of no other.
// adam (nullable; items with an update): the rule is Adam, not momentum SGD, for every item -- item i's second moments and the
// scalars every layer shares beyond PackItem's lr and mom (include/currennt_hip.h, cn_adam_update)
// clip (nullable; update == 1 items only): the record of grad_norm_kernel in front of the rule
// decay (nullable; items with an update): weight decay is on (include/currennt_hip.h, section Weight decay) and item i's
// ld = (float)(lr_layer * decay), for every update mode and behind clip
struct PackAdam { float *v[PACK_GROUP_MAX]; float b2, omb1, omb2, eps_t; };
struct ClipRecord;
struct PackDecayArgs { float ld[PACK_GROUP_MAX]; };
void launch_pack_group(hipStream_t s, bool f32, PackGroup &grp, hipEvent_t done = nullptr, const PackAdam *adam = nullptr, const ClipRecord *clip = nullptr,
                       const PackDecayArgs *decay = nullptr);
// Weight noise (include/currennt_hip.h, section Weight noise): the group's items name the NOISY copies in WinT / WrecT / peep_p
// (the launch writes nothing else) and the clean flat weights in w; item i's key word 0 is k0[i] = seed_lo + ordinal, the other
// key word (seed_hi ^ "nois"), counter words 2 and 3 and sigma are the group's.  Kernels of their own (pack_group_noise_kernel).
struct PackNoise { uint32_t k0[PACK_GROUP_MAX]; uint32_t k1, pass_lo, pass_hi; float sigma; };
void launch_pack_group_noise(hipStream_t s, bool f32, PackGroup &grp, const PackNoise &nz);
void launch_ff_pack(hipStream_t s, bool f32, const FfGeom &g, float bias, const float *w,
                    void *W, void *WT, float *bias_p);
void launch_ff_unpack_grads(hipStream_t s, const FfGeom &g, float bias, float *dW, float *colsum, float *wu, hipEvent_t done = nullptr);

// inputs [N][P] fp32 (reference layout) -> [N][Pp] op, zero padded
// rm (nullable): the fraction's row map, built behind the re-layout: rm[0] real frames, rm[1] dummy ones, rm[4 ..) the real rows in
// ascending order, rm[4 + maxN ..) the dummy rows
void launch_rowmap(hipStream_t s, const char *dpat, int N, int *rm, int maxN, int unchecked);    // rows < unchecked count as real
void launch_fraction_load(hipStream_t s, bool f32, int T, int PS, int PSp, const char *pat, char *dpat, const int *tcls, int *dtcls,
                          const float *tgt, float *dtgt, int W, const float *in, int P, void *dst, int Pp, int *rm = nullptr, int maxN = 0, int Tmin = 0);
void launch_pad_convert(hipStream_t s, bool f32, const float *src, int N, int P, void *dst, int Pp);
// ---- input augmentation (include/currennt_hip.h, section Input augmentation; cn_augment.hip) ----
// The settings of one re-layout as the kernels take them: P0 = P / (ctx_left + ctx_right + 1) features per frame, the two Philox
// keys ((seed_lo, seed_hi ^ "inpt") for the noise, (seed_lo, seed_hi ^ "mask") for the masks) and counter words 2 and 3.
// skip: the frame skip of a spliced load (section Input splicing and frame skipping): time t is network frame t, centred on
// source frame skip * t; 1 for every load that takes its fraction at network rate.
struct AugArgs {
    int P0, ctx_left, nfreq, fwidth, ntime, twidth, permille;
    uint32_t k0, k1_noise, k1_mask, pass_lo, pass_hi;
    float sigma;
    int skip;
};
#define AUG_MAX_MASKS 8                          // per kind
#define AUG_TAB_STRIDE (1 + 4 * AUG_MAX_MASKS)   // ints per slot: len, (start, width) of the frequency masks, then of the time masks
// tab[PS][AUG_TAB_STRIDE] from the pattern types pat[t * pstride + s] (0 <= t < T, 0 <= s < PS): one small workgroup
void launch_augment_table(hipStream_t s, const AugArgs &a, const char *pat, int pstride, int T, int PS, int *tab);
// launch_fraction_load with the augmentation of `a` / `tab` applied to the inputs on the way
void launch_fraction_load_augment(hipStream_t s, bool f32, const AugArgs &a, const int *tab, int T, int PS, int PSp, const char *pat, char *dpat,
                                  const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P, void *dst, int Pp,
                                  int *rm = nullptr, int maxN = 0, int Tmin = 0);
// launch_pad_convert of inputs already in the device's row layout (src[T * PSp][P], dpat[T * PSp]), with the same augmentation
void launch_pad_convert_augment(hipStream_t s, bool f32, const AugArgs &a, const int *tab, const float *src, const char *dpat, int T, int PS, int PSp,
                                int P, void *dst, int Pp);
// ---- input splicing and frame skipping (include/currennt_hip.h, section of that name; cn_splice.hip) ----
// The re-layout of a SOURCE-rate fraction (Tsrc steps of unspliced P0-wide patterns, host layout [Tsrc][PS]) into the Tnet =
// ceil(Tsrc / a.skip) network-rate steps of the padded device layout: derived pattern types, the classes / target rows of source
// row skip * j, the gathered inputs (P = B * P0 columns; through augment_value when `augment`), then the row map.  `tab` is
// launch_augment_table's for the source pattern types (row[0] = len_s is all an un-augmented load uses of it); a.P0, a.ctx_left
// and a.skip are read whether `augment` or not.
void launch_fraction_load_splice(hipStream_t s, bool f32, const AugArgs &a, bool augment, const int *tab, int Tnet, int PS, int PSp,
                                 char *dpat, const int *tcls, int *dtcls, const float *tgt, float *dtgt, int W, const float *in, int P,
                                 void *dst, int Pp, int *rm, int maxN, int Tmin_net);
// ---- dropout on a layer's input (include/currennt_hip.h, section Dropout) ----
// The key of one forward pass of one layer, and the geometry that maps a padded element to the reference (frame, unit) the mask
// is stated in: row r = t * PSp + ps <-> frame n = t * PS + ps (pad slots ps >= PS: zeros); column -> unit by the map of the rows
struct DropArgs {
    int N, PS, PSp; UnitMap prev;
    uint32_t k0, k1, pass_lo, pass_hi, thr;    // Philox key ((seed_lo + ordinal), seed_hi), counter words 2 and 3, keep threshold
    float scale;
};
// dst[N][Pp] (op) = masked, rescaled src[N][Pp] (op); pad rows and pad columns are written as zeros
void launch_dropout_fwd(hipStream_t s, bool f32, const DropArgs &a, const void *src, void *dst);
// err[N][Pp] (fp32) masked and rescaled in place with the same key
void launch_dropout_bwd(hipStream_t s, const DropArgs &a, float *err);
// ---- layer normalization of a layer's input (include/currennt_hip.h, section Layer normalization; cn_layernorm.hip) ----
// The geometry of one forward pass of one marked layer: N = T * PSp rows of the preceding layer's map.  PS / PSp: slots per time
// step without and with pad slots (what the debug hook unpads with).
struct LnArgs {
    int N, PS, PSp; UnitMap prev;
    float eps;
};
// (Pp = prev.Lp)  xn[N][Pp] (op) = the normalised x[N][Pp] (op) on the rows with pat[row] != 0, zeros on the other rows (dummy frames, pad slots)
// and in pad columns; rstd[N]: 1 / sqrt(var + eps) of every real row as a float, 0 elsewhere
void launch_layernorm_fwd(hipStream_t s, bool f32, const LnArgs &a, const char *pat, const void *x, void *xn, float *rstd);
// err[N][Pp] (fp32), dL/d xn, rewritten in place as dL/dx from the forward pass's xn and rstd; zeros on the rows with pat[row] == 0
void launch_layernorm_bwd(hipStream_t s, bool f32, const LnArgs &a, const char *pat, const void *xn, const float *rstd, float *err);
// ---- residual connections (include/currennt_hip.h, section Residual connections; cn_residual.hip) ----
// The geometry of one forward pass of one marked layer: N = T * PSp rows; the marked layer's own map and the preceding layer's,
// of the same L units (Lp = own.Lp, xLp = prev.Lp below).  same_map: unit u has the same column in both (the 16-byte path).
struct ResArgs {
    int N; UnitMap own, prev; int same_map;
};
// sum[N][Lp] (op) = branch[N][Lp] (op) + x[N][xLp] (op), one rounding to the operand type, on the rows with pat[row] != 0;
// the branch on the other rows (dummy frames, pad slots); pad columns are written as zeros
void launch_residual_fwd(hipStream_t s, bool f32, const ResArgs &a, const char *pat, const void *branch, const void *x, void *sum);
// prev_err[N][xLp] (fp32) += e[N][Lp] (fp32) on the rows with pat[row] != 0, unit by unit
void launch_residual_bwd(hipStream_t s, const ResArgs &a, const char *pat, const float *e, float *prev_err);
// ---- context layers (include/currennt_hip.h, sections Context layers and Strided context layers; cn_context.hip) ----
// The geometry of one forward pass of one context layer: it reads Tin steps of its predecessor's (the PARENT's) time axis and
// writes Tout = ceil(Tin / S) steps of PSp slots; a plain layer has S = 1 and lies in the parent's axis (Tout == Tin), a layer
// with S > 1 owns the axis it writes in.  B = left + right + 1 blocks of the preceding layer's P = prev.L units in rows
// Lp = round_up(B * P, 32) wide, block b at columns [b * P, (b + 1) * P); xLp = prev.Lp below.  len[] below is always the parent
// axis's (len_s); the kernels form n_s = ceil(len_s / S), the real frames of a slot in the layer's own axis, from it.
struct ContextArgs {
    int Tin, Tout, PSp, B, left, dil, Lp, S; UnitMap prev;
};
// len[PSp]: the frames of every slot whose pattern type is not NONE, from pat[t * PSp + s], t < T (one wave per slot)
void launch_context_lengths(hipStream_t s, const char *pat, int T, int PSp, int *len);
// S > 1: the layer's own axis from the parent's, every row of Tout * PSp written: nlen[s] = n_s, the derived pattern types npat
// (FIRST / NORMAL / LAST / NONE) and the classes ntcls[j][s] = tcls[S * j][s] for j < n_s, -1 elsewhere
void launch_stride_axis(hipStream_t s, int S, int Tout, int PSp, const int *len, const int *tcls, int *nlen, char *npat, int *ntcls);
// tgt[Tout * PSp][W] = src[rate * j][s][..] for j < nlen[s], zero rows elsewhere (src at the base rate, rate = the product of the strides)
void launch_stride_targets(hipStream_t s, int rate, int Tout, int PSp, int W, const int *nlen, const float *src, float *tgt);
// out[Tout * PSp][Lp] (op) gathered from x[Tin * PSp][xLp] (op), bits copied; rows j >= n_s and pad columns are written as zeros
void launch_context_fwd(hipStream_t s, bool f32, const ContextArgs &a, const int *len, const void *x, void *out);
// dx[Tin * PSp][xLp] (fp32), every row and column written: the fold of e[Tout * PSp][Lp] (fp32) in the stated order, zeros elsewhere
void launch_context_bwd(hipStream_t s, const ContextArgs &a, const int *len, const float *e, float *dx);
// delta = act'(y) * err (in place on err, all N slots: FeedForwardLayer.cu:72-79), op copy for the GEMMs
void launch_ff_delta(hipStream_t s, bool f32, int act, const float *y, float *err, void *delta_op, int N, int L, int Lp);
// column sums of delta over the N slots (FeedForwardLayer.cu:82-102): colsum[j] += sum_n err[n][j]
// det_part (nullable; deterministic mode): det_colsum_part_floats(Lp) floats; the workgroups store their partial sums there and a
// second launch adds them in workgroup order
// fold_out (nullable): the fold is not launched but described there (nparts = 0: nothing to fold) for the caller to attach to
// the layer's gradient product (launch_gemm_tn's `extra`)
void launch_colsum(hipStream_t s, const float *err, int N, int Lp, float *colsum, float *det_part = nullptr, FoldItem *fold_out = nullptr);
size_t det_colsum_part_floats(int Lp);
// softmax rows in place (SoftmaxLayer.cu:250-315), dummies skipped
// optional: tcls + rowstat[N][2] = {log p_target, argmax == target} for the multiclass loss
// smstat (nullable, wide rows only: softmax_fwd_can_be_lazy): the LAZY form -- y keeps the logits, smstat[N][2] = {offset, sum};
// launch_softmax_mcc_bwd(.., smstat) and launch_softmax_normalise recompute the very same posteriors from them
// fast (wide rows only; the bf16 throughput mode): v_exp_f32 and one reciprocal per row in place of expf and a division per element
void launch_softmax_fwd(hipStream_t s, float *y, const char *pat, int N, int L, int Lp, const int *tcls, float *rowstat, bool fast = false, float *smstat = nullptr);
bool softmax_fwd_can_be_lazy(int L);
void launch_softmax_normalise(hipStream_t s, bool fast, float *y, const char *pat, int N, int L, int Lp, const float *smstat);
void launch_rowstat_reduce(hipStream_t s, const float *rowstat, int N, float *loss2, bool reset, float scale = -1.0f);
// remaining post output layers (row f4): per-pattern terms -> rowstat -> fixed-order sum
enum { POST_SSE = 0, POST_WEIGHTEDSSE, POST_SSE_MASK, POST_CE, POST_RMSE, POST_BINARY };
void launch_post_eval(hipStream_t s, int kind, const float *y, const float *tgt, const char *pat, int N, int L, int Lp,
                      float *rowstat, float *loss2, bool reset);
void launch_post_backward(hipStream_t s, int kind, const float *y, const float *tgt, const char *pat, int N, int L, int Lp, float *err);
void launch_classes_to_targets(hipStream_t s, const int *tcls, float *tgt, int N);
// multiclass error injection + softmax Jacobian + delta copy + bias column sums in one pass (Lp <= 256)
// rowstat / loss2 (nullable; narrow rows only, softmax_mcc_bwd_takes_loss): the launch also sums the forward pass's row
// statistics into loss2 like launch_rowstat_reduce(..., reset = false) would (the same sums in the same order), in sixteen extra workgroups
// `loss_part`: 16 x {float sum, int count} + one arrival counter (zero between launches) for the sixteen reduction workgroups
void launch_softmax_mcc_bwd(hipStream_t s, bool f32, const float *y, const int *tcls, const char *pat, int N, int L, int Lp,
                            float *err, void *delta_op, float *colsum, const float *rowstat = nullptr, float *loss2 = nullptr, float *loss_part = nullptr,
                            const float *smstat = nullptr, bool fast = false, float *colpart = nullptr, float *det_part = nullptr, FoldItem *fold_out = nullptr);
bool softmax_mcc_bwd_takes_loss(int Lp);
// `colpart` (nullable; narrow rows): softmax_mcc_bwd_colpart_floats() zeroed floats the launch spreads its column-sum atomics over
// (replicas folded into colsum by the last workgroup; zero again when the launch ends)
size_t softmax_mcc_bwd_colpart_floats();
// e_i <- y_i (e_i - sum_j y_j e_j) (SoftmaxLayer.cu:317-349), dummies skipped
void launch_softmax_bwd(hipStream_t s, const float *y, float *err, const char *pat, int N, int L, int Lp);
// multiclass_classification: loss/#correct reduction and error injection
// rowstat: [N][2] scratch the per-pattern terms pass through (summed in a fixed order: launch_rowstat_reduce)
void launch_mcc_eval(hipStream_t s, const float *y, const int *tcls, int N, int L, int Lp, float *loss2 /*[2]*/, bool reset, float *rowstat);
void launch_mcc_backward(hipStream_t s, const float *y, const int *tcls, int N, int L, int Lp, float *err);
// sse
// UpdateWeightFn over a flat range
void launch_scale(hipStream_t s, float *x, size_t n, float a);     // x *= a
// dst[i] = src[0][i] + src[1][i] + ... in that order (cn_comm_ipc.cpp: the test backend of the gradient exchange)
struct SumRanks { const float *src[8]; int n; };
void launch_sum_ranks(hipStream_t s, float *dst, const SumRanks &sr, size_t n);

// ---- CN_COMM_BACKEND=ipc: test backend of cn_comm_* for ranks that share a device (cn_comm_ipc.cpp) ----------------
struct IpcComm;
bool ipc_backend_selected();
void ipc_unique_id(char *id, size_t bytes);
IpcComm *ipc_comm_create(const char *id, int rank, int world);
void ipc_comm_destroy(IpcComm *c);
void ipc_comm_mark_failed(IpcComm *c);
void ipc_allreduce(IpcComm *c, float *buf, size_t n, hipStream_t st, size_t capacity_hint = 0);
bool ipc_comm_is_p2p(const IpcComm *c);
void ipc_comm_check(IpcComm *c, hipStream_t st);       // p2p: raise if a poll of the communicator timed out (synchronises st)
void ipc_comm_check_fast(IpcComm *c);                  // p2p: the same from the host-mapped word the kernel sets (no synchronisation)
// p2p: allocate and map the regions and run the first-contact self-check (flags and staged lines through every peer's mapping,
// both forms of the exchange, sums verified on the host).  False: some rank saw a wrong sum or a time-out -- every rank gets the
// same answer -- and `rccl_id` (CN_COMM_ID_BYTES) holds what rank 0's `make_id` produced: the caller fails over to RCCL.
bool ipc_comm_p2p_selfcheck(IpcComm *c, hipStream_t st, void (*make_id)(char *), char *rccl_id);
void ipc_allreduce_loss(IpcComm *c, float *err, int *correct);
// ---- CN_COMM_BACKEND=p2p: one stream-ordered kernel per bucket over peer-mapped regions (cn_comm_p2p.hip) -----------
constexpr int P2P_GROUPS = 64, P2P_THREADS = 256;
// a rank's region starts with 64-bit flag words: [word][source rank][workgroup]
constexpr int P2P_READY = 0, P2P_REDUCED = 8 * P2P_GROUPS, P2P_DONE = 16 * P2P_GROUPS, P2P_FAILED = 24 * P2P_GROUPS, P2P_FLAG_WORDS = 24 * P2P_GROUPS + 64;
struct P2pArgs {
    float *buf; size_t n, piece, slot;         // the bucket (in place); floats per piece (even): n <= world * P2P_GROUPS * piece; per staging slot (>= piece)
    float *stage[8];                           // staging half of this exchange, per rank (peers' mapped into this process)
    unsigned long long *flags[8];              // flag words, per rank
    int me, world, two_phase;
    unsigned long long seq, timeout_ticks;     // exchange counter (from 1); poll deadline in ticks of the 100 MHz clock
    unsigned long long *host_failed;           // host-mapped word: set when a wait of this exchange ended without its flag
};
void launch_p2p_allreduce(hipStream_t s, const P2pArgs &a);
void launch_accumulate(hipStream_t s, float *acc, const float *wu, size_t n, bool first);

// ---- global gradient-norm clipping (include/currennt_hip.h, section Gradient clipping) ----
// The sum of squares runs over CLIP_LANES strided lanes (lane k: g[k]^2, g[k + L]^2, ... in ascending order, in double), then a
// tree over NEIGHBOURING lanes.  A thread of grad_norm_kernel owns four neighbouring lanes (one 16-byte load per row), a
// workgroup 1024, so the tree's first two levels are a thread's registers, the next eight the workgroup's LDS and the last four
// the CLIP_WGS workgroup sums, which the last workgroup to arrive adds.
constexpr int CLIP_LANES = 16384, CLIP_WGS = 16;
enum { CLIP_NONE = 0, CLIP_SCALE = 1, CLIP_SKIP = 2 };
// The device record of a context with clipping on (zeroed at allocation).  {norm, scale, state} is what the update launches
// that follow read; the counters are the finishing thread's; part / arrivals belong to the hand-off (arrivals is zero between
// launches).
struct ClipRecord {
    float norm, scale; int state; float max_seen;
    long long updates, clipped, skipped;
    unsigned arrivals, pad;
    double part[CLIP_WGS];
};
// one pass over g[0 .. n) (n a multiple of 4, g 16-byte aligned: the weightUpdates part of the arena); fills *rec
void launch_grad_norm(hipStream_t s, const float *g, size_t n, float max_norm, ClipRecord *rec);

// ---- the flat update: one launch over a range [0, n) of the arena (flat_update_kernel) ----
// The range and momentum SGD's scalars: wd the weight deltas.  Under Adam (adam given) wd holds the first moments, and lr and mom
// are not read: FlatAdam has the range's second moments and the step's scalars (one block, as adam_scalars forms them)
struct FlatUpdate { float *w; const float *wu; float *wd; size_t n; float lr, mom; };
struct AdamScalars { float b1, omb1, b2, omb2, alpha_t, eps_t; };      // (include/currennt_hip.h, cn_adam_update)
struct FlatAdam { float *v; AdamScalars a; };
// Weight decay (include/currennt_hip.h, section Weight decay): the range is ONE layer's, and w0 = w - ld * w is in front of the
// rule for the entries of [0, a1) and [b0, b1) (the input weights and an LSTM layer's recurrent weights)
struct DecayRanges { size_t a1, b0, b1; };
struct FlatDecay { float ld; DecayRanges rg; };
// adam, clip, decay (each nullable): the launch's features, as launch_pack_group's; clip: g' = scale * g on CLIP_SCALE, nothing
// touched on CLIP_SKIP.  256 threads, min(ceil(n / 256), 2048) workgroups, nothing launched for n == 0; done rides on the launch.
void launch_flat_update(hipStream_t s, const FlatUpdate &u, const FlatAdam *adam = nullptr, const ClipRecord *clip = nullptr,
                        const FlatDecay *decay = nullptr, hipEvent_t done = nullptr);

// ---- LAMB (include/currennt_hip.h, section LAMB; cn_lamb.hip) ----
// The host scalars of the section, and the context's decay coefficient and trust bounds (max_ratio 0: no upper bound)
struct LambScalars { float b1, omb1, b2, omb2, c_t, eps_t, decay, min_ratio, max_ratio; };
// One layer of a launch: its range of the arena (off floats in, n = the padded count), the runs of it that decay ([0, a1) and
// [b0, b1), relative to off), its effective rate and its record's index
struct LambItem { size_t off; unsigned n, a1, b0, b1; float lr; int rec; };
constexpr int LAMB_GROUP_MAX = 16;
struct LambGroup { LambItem item[LAMB_GROUP_MAX]; int n; };
// rows of CLIP_LANES entries a thread of lamb_direction_kernel loads in front of its dependent adds; the grid of lamb_apply_kernel
constexpr int LAMB_UNROLL = 4;
constexpr unsigned LAMB_APPLY_MAX_BLOCKS = 256;
// A layer's device record: what its last LAMB step found (ratio 1, norms 0 before the first); part_* / arrivals belong to the
// hand-off (arrivals is zero between launches)
struct LambRecord {
    float nw, nu, ratio; unsigned arrivals;
    double part_w[CLIP_WGS], part_u[CLIP_WGS];
};
// One direction launch and one apply launch over the group's layers: m = arena + 2 * total, g = arena + total, v and u are [total]
// like a part of the arena.  clip (nullable): the clipping record in front of the rule; done rides on the apply launch.
void launch_lamb(hipStream_t s, const LambGroup &grp, float *arena, size_t total, float *v, float *u, const LambScalars &a, LambRecord *recs,
                 const ClipRecord *clip = nullptr, hipEvent_t done = nullptr);

// ---- weight averaging (include/currennt_hip.h, section Weight averaging; cn_average.hip) ----
// avg[0 .. n) = copy ? w : avg + omd * (w - avg), every operation an fp32 operation rounded on its own (n a multiple of 4, both
// pointers 16-byte aligned: the weights part of the arena and the context's average)
void launch_weight_average(hipStream_t s, float *avg, const float *w, size_t n, float omd, bool copy);
// w[0 .. n) <-> avg[0 .. n)
void launch_weight_swap(hipStream_t s, float *w, float *avg, size_t n);

// ---- CTC post output layer (cn_ctc.hip; the arithmetic is stated in that file's header) -----------------------------------------
struct CtcArgs {
    const float *y; const char *pat;      // posteriors [T * PSp][Lp], pattern types [T * PSp]
    int T, PSp, C, Lp;
    // label sequences in slot order: slot s owns entries laboff[s] .. laboff[s + 1) (laboff has PSp + 1 entries; empty and pad
    // slots own none); next[u]: the next position of the same slot with the same label, relative to laboff[s], or -1;
    // first[u]: no earlier position of the slot has this label
    const int *labels, *next, *first, *laboff;
    int maxS;                             // 2 * (longest label sequence of the fraction) + 1
    int2 *alpha, *beta; int Sp;           // the sweeps' columns, [PSp][T][Sp] pairs {mantissa bits, exponent} each, Sp >= maxS
    int *info;                            // [PSp][2]: {len, 1 if the sequence has an alignment with p > 0}
    float *rowstat;                       // [PSp][2]: slot s receives {-log p, 1} or {0, 0}
    float *err;                           // [T * PSp][Lp] dL/dy (launch_ctc_errors)
    int only;                             // launch_ctc_sweeps sets it: 0 both sweeps in this launch (blockIdx.y), 1 alpha alone, 2 beta alone
};
constexpr int CTC_MAX_STATES = 4096;      // sixteen states per thread of a 256-thread workgroup
// can a layer with this label cap and output pitch run (states per workgroup, LDS of the error kernel)?
bool ctc_shape_fits(int max_labels, int Lp);
// alpha and beta sweeps of every slot, concurrently (option ctc_serial_sweeps: two launches, one behind the other); fills alpha,
// beta, info and rowstat
void launch_ctc_sweeps(hipStream_t s, const CtcArgs &a);
// behind the sweeps: every row and column of err
void launch_ctc_errors(hipStream_t s, const CtcArgs &a);

// ---- CTC decoding (cn_ctc_decode.hip; the rule is stated in that file's header) --------------------------------------------------
struct CtcDecodeArgs {
    const char *pat; int T, PSp, C;       // pattern types [T * PSp] of the ctc layer's own time axis
    const int *amax;                      // [T * PSp] launch_ctc_argmax's result
    const int *labels, *laboff;           // as CtcArgs; laboff == nullptr: the fraction has no labels, every distance is -1
    int maxShort;                         // >= min(D, U) of every slot: min(T, longest label sequence of the fraction)
    int *decoded, *decoded_len, *dist;    // [PSp][T], [PSp], [PSp]
    unsigned long long *sums;             // {label errors, labels}: added to, or nullptr
};
constexpr int CTC_ARGMAX_WAVE_C = 1024;   // up to this many units a wave takes a row, above it a workgroup
constexpr int CTC_DECODE_MAX_SHORT = 5119;   // three diagonals of maxShort + 1 ints in 60 KB of LDS
bool ctc_decode_fits(int T, int max_labels);
// amax[n] = index of the largest of y[n][0 .. C), the lowest of equal ones; -1 for a row with pat[n] == 0
void launch_ctc_argmax(hipStream_t s, const float *y, const char *pat, int N, int C, int Lp, int *amax);
// behind it: decoded, decoded_len, dist and, if asked for, the sums
void launch_ctc_collapse(hipStream_t s, const CtcDecodeArgs &a);
// gather a padded row-major fp32/op matrix into the reference layout [N][L]
// (host row n = t*PS + s maps to device row t*PSp + s)
void launch_unpad(hipStream_t s, bool src_is_bf16, const void *src, long ld, int col0, int cstride, int N, int L, float *dst, long ldd, int dcol0, int PS, int PSp);
// scatter host-provided [N][m.L] fp32 into the padded fp32 rows of map m (tests)
void launch_pad_f32(hipStream_t s, const float *src, int N, float *dst, const UnitMap &m, int PS, int PSp);

}  // namespace cn
