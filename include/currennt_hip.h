/*
 * currennt_hip.h -- C ABI of libcurrennt_hip.so, the MI355X (gfx950) implementation of the
 * CURRENNT LSTM training hot path (naxingyu/lstm-rnn, currennt_lib/src).
 *
 * The reference has no FFI layer: its seam is the virtual layers::Layer<TDevice> interface
 * (layers/Layer.hpp:40-179, layers/TrainableLayer.hpp:84-155, layers/PostOutputLayer.hpp:80)
 * plus the GEMM seam helpers::Matrix / helpers::cublas::multiplyMatrices
 * (helpers/Matrix.hpp:48-49, helpers/cublas.hpp:30-38).  Every entry point below names the
 * reference method it stands in for; a maintainer binds them from a `Hip` device policy next to
 * `Cpu`/`Gpu` (Types.hpp:45-67) as shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handles, ints, floats, raw pointers; no C++ or torch types.
 *   - every function returns 0 on success or a negative cn_status; the message is available
 *     from cn_last_error() (the reference throws std::runtime_error(msg), e.g. Matrix.cu:209-210;
 *     host wrappers turn a non-zero status back into an exception -> "FAILED: msg", exit code 2,
 *     main.cpp:492-495).
 *   - host arrays use the reference layouts: activations [t*PS + ps][unit]
 *     (DataSet.cpp:359,376,383,406), flat weight vectors as in LstmLayer.hpp:36-55 and
 *     FeedForwardLayer.cu:148,160.  Padded / packed / bf16 device copies are internal.
 *   - one cn_ctx per GPU, used from one host thread at a time (the reference is single-threaded,
 *     cublas.cu:33-43).  All work is enqueued on the ctx stream; only the functions marked
 *     [sync] wait for the device.
 */
#ifndef CURRENNT_HIP_H
#define CURRENNT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cn_ctx   cn_ctx;
typedef struct cn_layer cn_layer;

typedef enum cn_status {
    CN_OK            =  0,
    CN_ERR_BAD_ARG   = -1,   /* null handle, negative size, unknown enum                     */
    CN_ERR_SHAPE     = -2,   /* size mismatch (reference: "Invalid matrix dimensions", ...)  */
    CN_ERR_HIP       = -3,   /* a HIP runtime call failed                                    */
    CN_ERR_STATE     = -4,   /* call order violated (e.g. forward before a fraction is loaded)*/
    CN_ERR_NO_DEVICE = -5,   /* no gfx950 device / code object cannot run here               */
    CN_ERR_COMM      = -6    /* RCCL could not be loaded / a collective call failed            */
} cn_status;

/* arithmetic mode of the GEMM operands (accumulation and all state are always fp32) */
typedef enum cn_precision {
    CN_PREC_F32    = 0, /* fp32 operands on v_mfma_f32_*_f32: exact-fp32 parity mode (real_t = float, Types.hpp:39); the fp32
                           MFMAs run at 1/16 of the bf16 rate                                                              */
    CN_PREC_BF16   = 1, /* bf16 operands on v_mfma_f32_*_bf16: throughput mode                                            */
    CN_PREC_BF16X3 = 2  /* fp32 operands in memory, every operand split into bf16 hi + bf16 lo inside the kernels and a product
                           computed as three bf16 MFMAs (hi*hi + lo*hi + hi*lo, fp32 accumulation): ~2^-16 relative per term,
                           i.e. the fp32 tolerance of BASELINE.json (posterior max-abs < 1e-4) at a third of the bf16 MFMA rate --
                           the parity mode that is fast; state, activations and gradients sums are fp32 as in the other modes      */
} cn_precision;

/* layer kinds = the type strings of LayerFactory.cu:52-87 that are on the hot path */
typedef enum cn_layer_kind {
    CN_LAYER_INPUT = 0,                   /* "input"                      InputLayer.cpp            */
    CN_LAYER_LSTM,                        /* "lstm"                       LstmLayer.cu              */
    CN_LAYER_BLSTM,                       /* "blstm"                      LstmLayer.cu              */
    CN_LAYER_FF_TANH,                     /* "feedforward_tanh"           FeedForwardLayer.cu       */
    CN_LAYER_FF_LOGISTIC,                 /* "feedforward_logistic"                                 */
    CN_LAYER_FF_IDENTITY,                 /* "feedforward_identity"                                 */
    CN_LAYER_SOFTMAX,                     /* "softmax"                    SoftmaxLayer.cu           */
    CN_LAYER_SSE,                         /* "sse"                        SsePostOutputLayer.cu     */
    CN_LAYER_MULTICLASS_CLASSIFICATION,   /* "multiclass_classification"  MulticlassClassificationLayer.cu */
    /* remaining post output layers of LayerFactory.cu:52-87.  The weighted kinds have size == 2 * size of
     * the output layer and take interleaved (target, weight | filter input) pairs in cn_fraction.targets;
     * binary_classification has size 1 and reads cn_fraction.target_classes. */
    CN_LAYER_WEIGHTEDSSE,                 /* "weightedsse"                WeightedSsePostOutputLayer.cu    */
    CN_LAYER_SSE_MASK,                    /* "wf"                         SseMaskPostOutputLayer.cu        */
    CN_LAYER_CE,                          /* "ce"                         CePostOutputLayer.cu             */
    CN_LAYER_RMSE,                        /* "rmse"                       RmsePostOutputLayer.cu           */
    CN_LAYER_BINARY_CLASSIFICATION,       /* "binary_classification"      BinaryClassificationLayer.cu     */
    /* Connectionist Temporal Classification (Graves et al. 2006; no counterpart in the reference): behind a softmax layer of the
     * same size (>= 2) whose LAST unit is the blank.  It reads nothing from cn_fraction.target_classes / targets (and
     * output_pattern_size is not checked against it); its targets are label sequences, cn_layer_set_label_sequences below. */
    CN_LAYER_CTC,                         /* "ctc"                        csrc/cn_ctc.hip                  */
    /* Above: the kinds cn_layer_create takes.  Behind them, on this line so that the list of those kinds still ends with ctc: a
     * hidden layer that splices its predecessor's neighbouring frames (no counterpart in the reference), created by
     * cn_layer_create_context alone, section Context layers below; csrc/cn_context.hip */ CN_LAYER_CONTEXT
} cn_layer_kind;

/* which device vector cn_layer_read / cn_layer_device_ptr addresses */
typedef enum cn_buffer {
    CN_BUF_OUTPUTS = 0,        /* Layer::outputs()               [N][size]  Layer.hpp:132        */
    CN_BUF_OUTPUT_ERRORS,      /* Layer::outputErrors()          [N][size]  Layer.hpp:153        */
    CN_BUF_WEIGHTS,            /* TrainableLayer::weights()      flat       TrainableLayer.hpp:119*/
    CN_BUF_WEIGHT_UPDATES,     /* TrainableLayer::weightUpdates() flat      TrainableLayer.hpp:133*/
    CN_BUF_WEIGHT_DELTAS,      /* SteepestDescentOptimizer::m_weightDeltas  SteepestDescentOptimizer.cu:117-123 */
    /* LSTM per-direction internals, [N][H] each (LstmLayer.hpp:88-100,170-233); `dir` selects fw/bw */
    CN_BUF_LSTM_CELL_STATES,
    CN_BUF_LSTM_NI_ACTS,
    CN_BUF_LSTM_IG_ACTS,
    CN_BUF_LSTM_FG_ACTS,
    CN_BUF_LSTM_OG_ACTS,
    CN_BUF_LSTM_NI_DELTAS,
    CN_BUF_LSTM_IG_DELTAS,
    CN_BUF_LSTM_FG_DELTAS,
    CN_BUF_LSTM_OG_DELTAS,
    CN_BUF_LSTM_TMP_OUTPUTS,   /* per-direction block outputs y */
    /* Adam's second moments v, flat like the weights (cn_adam_update below; no counterpart in the reference, whose only optimizer
     * state is m_weightDeltas, SteepestDescentOptimizer.cu:117-123).  Valid in cn_layer_read / cn_layer_upload /
     * cn_layer_device_ptr; a read before any Adam call returns zeros.  Adam's FIRST moments are CN_BUF_WEIGHT_DELTAS. */
    CN_BUF_ADAM_SECOND_MOMENTS
} cn_buffer;

/* one parallel-sequence mini batch = data_sets::DataSetFraction (DataSetFraction.hpp:50-60) */
typedef struct cn_fraction {
    int          max_seq_length;    /* T     = fraction.maxSeqLength()                               */
    int          min_seq_length;    /* Tmin  = fraction.minSeqLength()                               */
    int          num_sequences;     /* fraction.numSequences() (<= parallel_sequences)               */
    int          input_pattern_size;/* fraction.inputPatternSize()                                   */
    int          output_pattern_size;/* fraction.outputPatternSize()                                  */
    const char  *pat_types;         /* [T*PS]            0 = PATTYPE_NONE  (Types.hpp:30-33)         */
    const float *inputs;            /* [T*PS][inputSize]                                              */
    const int   *target_classes;    /* [T*PS] or NULL    -1 on dummy slots (DataSet.cpp:336)         */
    const float *targets;           /* [T*PS][outputSize] or NULL                                     */
} cn_fraction;

/* ---- context ------------------------------------------------------------------------------- */

/* Replaces the device selection of main.cpp:526-541 and the lazy cuBLAS handle of cublas.cu:33-43.
 * `stream` is a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream) or NULL
 * for a stream owned by the context. */
int  cn_ctx_create(int device_id, cn_precision precision, void *stream, cn_ctx **out);
int  cn_ctx_destroy(cn_ctx *ctx);
int  cn_ctx_synchronize(cn_ctx *ctx);                                   /* [sync] */
/* Named integer options of a context (no counterpart in the reference, whose Cpu path has nothing to choose):
 *   "deterministic"  1: every sum over the patterns of a fraction -- weight gradients (ComputeWeightUpdateFn,
 *                    LstmLayer.cu:289-512; FeedForwardLayer.cu:82-102,200-207), bias / peephole / column sums, the error --
 *                    is formed in a fixed order (partials stored by their producers, added by one thread per output), so
 *                    two runs on the same inputs give BIT-IDENTICAL gradients and weights, like the reference's serial
 *                    sums.  0: fp32 atomics in arrival order.  Default: 1 for CN_PREC_F32 / CN_PREC_BF16X3 (the parity
 *                    modes), 0 for CN_PREC_BF16; the environment variable CN_DETERMINISTIC=0/1 sets the default.
 *   "overlap"        1 (default): weight-gradient products on side streams beside the recurrent kernels; 0: one stream.
 *   A/B and test switches of the kernel selection (csrc/cn_internal.h, CN_OPTION_LIST; e.g. "no_s2_asm", "no_cluster",
 *                    "no_big_tn", "tnbig_group_mink", "lazy_softmax"): every one of them was an environment variable read
 *                    somewhere on a launch path until round 5.  Now the environment (CN_<NAME>) is read ONCE, at
 *                    cn_ctx_create, into the context's options block; this call changes an entry afterwards; no launch path
 *                    calls getenv.  Options that size allocations ("cluster4", "no_cluster") belong before the layers.
 * Unknown names fail with CN_ERR_BAD_ARG.  May be changed between fractions.                                       */
int  cn_ctx_set_option(cn_ctx *ctx, const char *name, int value);
int  cn_ctx_get_option(const cn_ctx *ctx, const char *name, int *value);
/* The weight-gradient GEMMs of a backward pass run on an internal side stream beside the next layer's
 * recurrent kernel.  Every entry point of this library orders itself behind them; call cn_ctx_join before
 * ANOTHER library (e.g. RCCL through torch.distributed) reads weightUpdates on the ctx stream: it makes the
 * ctx stream wait (device-side, no host sync) for the side stream. */
int  cn_ctx_join(cn_ctx *ctx);
/* The same for the weightUpdates of ONE layer: the context's stream waits for that layer's gradient work only.
 * Lets a data-parallel caller all-reduce the gradient of layer k+1 while layer k is still in its backward
 * pass (SURVEY.md 8e "Overlap": bucket = layer).  No-op when nothing is pending for the layer.   [async] */
int  cn_layer_join(cn_layer *layer);
/* The HIP stream (hipStream_t) the context enqueues its work on: the one given to cn_ctx_create, or the
 * library's own.  For callers that order foreign work (a collective library's stream) against it. */
void *cn_ctx_stream(cn_ctx *ctx);
/* The same ordering for a stream of the CALLER's choice (a HIP stream handle): `stream` waits for the gradient work
 * of `layer` and for nothing else the context has enqueued since, so a collective issued on it can start while the
 * context's stream is still busy with the backward pass of the layers below.  The caller orders the context's
 * stream behind that collective before the next cn_sgd_update*.                                      [async] */
int  cn_layer_join_stream(cn_layer *layer, void *stream);
/* message of the last failed call on this thread (ctx may be NULL for creation failures) */
const char *cn_last_error(cn_ctx *ctx);
/* "gfx950" etc. of the bound device; version string of the library */
const char *cn_device_arch(cn_ctx *ctx);
/* Device enumeration for `--list_devices` (main.cpp:509-525: cudaGetDeviceCount / cudaGetDeviceProperties).
 * cn_device_count returns the number of HIP devices (0 when there is none); cn_device_name copies the name of
 * device `index` ("<marketing name> (<gfx arch>)") into `buf` and returns a status. */
int  cn_device_count(void);
int  cn_device_name(int index, char *buf, int buf_size);
const char *cn_version(void);

/* ---- layers (LayerFactory<TDevice>::createLayer, LayerFactory.hpp:49-56) -------------------- */

/* `preceding` is NULL only for CN_LAYER_INPUT.  parallel_sequences / max_seq_length size every
 * buffer once, as Layer.cpp:59-66 and LstmLayer.cu:553-574 do; they are taken from `preceding`
 * for all other layers (pass 0).  `bias` is the JSON "bias" value (TrainableLayer.cu:57). */
int  cn_layer_create(cn_ctx *ctx, cn_layer_kind kind, cn_layer *preceding, int size, float bias,
                     int parallel_sequences, int max_seq_length, cn_layer **out);
int  cn_layer_destroy(cn_layer *layer);

int  cn_layer_size(const cn_layer *layer);
int  cn_layer_kind_of(const cn_layer *layer);
/* number of weights: size*(inputWeightsPerBlock*(P+1)+internalWeightsPerBlock), TrainableLayer.cu:101 */
int  cn_layer_weight_count(const cn_layer *layer);

/* Layer::loadSequences(fraction) for every layer of the stack: uploads patTypes once (the
 * reference copies them per layer, Layer.cpp:140), inputs (InputLayer.cpp:49-60) and targets /
 * target classes (PostOutputLayer.cpp:67-79, MulticlassClassificationLayer.cu:186-192).
 * Error texts follow the reference ("Input layer size of X != data input pattern size of Y").
 * The host buffers of `fraction` may be reused as soon as the call returns (they are copied into pinned staging
 * memory; the upload itself and the re-layout kernel are asynchronous).                                [async] */
int  cn_fraction_load(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *fraction);

/* The same with every pointer of `fraction` addressing DEVICE memory of the context's GPU (inputs already
 * resident in HBM: a prefetching data loader uploads fraction k+1 while fraction k trains).  Copies are
 * device-to-device on the ctx stream; nothing synchronises. */
int  cn_fraction_load_resident(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *fraction);

/* Announces the fraction the NEXT cn_fraction_load_resident will load (same descriptor, same layers).  The library
 * re-lays it out into a second set of buffers on the side stream of the next gradient work -- beside the backward
 * pass of the current fraction -- and that load then only exchanges the buffers (no kernel, nothing on the critical
 * path).  Purely a hint: a load of any other fraction, a host-buffer load, or a backward pass that put nothing on
 * the side stream simply discards it and loads the ordinary way.  The device buffers of `fraction` must stay
 * unchanged until that load.  CN_ERR_STATE
 * when a prefetch that is already in flight has not been consumed.  The reference has no counterpart (its loader
 * thread prefetches HOST fractions, DataSet.cpp:546-552; Layer::loadSequences copies synchronously).   [async] */
int  cn_fraction_prefetch_resident(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *fraction);
/* The same for HOST buffers: announces the fraction the NEXT cn_fraction_load will load.  The library packs it into pinned
 * staging memory and starts its upload at once (copy stream), re-lays it out beside the coming backward pass, and that load
 * only exchanges buffers -- what the reference's loader thread does for host fractions one fraction ahead (DataSet.cpp:202-
 * 240,546-552,589), moved across PCIe as well.  The caller's buffers are copied before this returns.  Purely a hint, as above.
 * CN_ERR_STATE when a prefetch that is already in flight has not been consumed.   [async] */
int  cn_fraction_prefetch(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *fraction);

/* Layer::computeForwardPass / computeBackwardPass (Layer.hpp:165-170).  Backward of a trainable
 * layer consumes its outputErrors, writes the preceding trainable layer's outputErrors
 * (LstmLayer.cu:990-1009, FeedForwardLayer.cu:188-198) and its own weightUpdates. */
int  cn_layer_forward(cn_layer *layer);
int  cn_layer_backward(cn_layer *layer);

/* The label sequences of the fraction loaded last, for a CN_LAYER_CTC layer: `labels` holds the sequences of slots
 * 0 .. num_sequences-1 one behind the other, label_lengths[s] labels for slot s, every label in [0, size - 2] (size - 1 is the
 * blank).  num_sequences must equal the loaded fraction's.  Both host arrays are copied before the call returns; the upload is
 * ordered on the context's stream.  The labels belong to that fraction: every cn_fraction_load* (a prefetch hit included)
 * invalidates them, and cn_loss_eval / cn_loss_accumulate / cn_layer_backward of a ctc layer without labels fail with
 * CN_ERR_STATE.  A label outside the range, a negative length or another num_sequences: CN_ERR_BAD_ARG.  A sequence longer than
 * the layer's cap -- min(max_seq_length, 512) labels, or the context option "ctc_max_labels" as it stood when the layer was
 * created (it sizes the workspace) -- : CN_ERR_SHAPE.
 * The error of a fraction is the sum of -log p(labels | inputs) over its sequences.  A sequence without an alignment (length 0, or
 * more labels + adjacent repeats than frames) contributes 0 and gets zero output errors.                          [async] */
int  cn_layer_set_label_sequences(cn_layer *ctc, const int *labels, const int *label_lengths, int num_sequences);

/* PostOutputLayer::calculateError() and, for multiclass_classification,
 * countCorrectClassifications() (MulticlassClassificationLayer.cu:159-177,194-213).
 * `correct` may be NULL; it is set to -1 for layers without a class count.  For a ctc layer it is the number of sequences
 * that contributed to the error (those with an alignment), and so is the count cn_loss_accumulate adds.        [sync] */
int  cn_loss_eval(cn_layer *post_output, float *error, int *correct);

/* Asynchronous form for the training loop: add this fraction's error / #correct to device-side
 * accumulators (Optimizer.cu:46-55 sums them per epoch on the host, two blocking D2H copies per
 * fraction) and read the sums once with cn_loss_read ([sync]; `reset` != 0 clears them). */
int  cn_loss_accumulate(cn_layer *post_output);
int  cn_loss_read(cn_ctx *ctx, float *error_sum, int64_t *correct_sum, int reset);

/* ---- weights (TrainableLayer.cu:65-101,211-248) --------------------------------------------- */

int  cn_layer_set_weights(cn_layer *layer, const float *host, int count);       /* flat reference layout */
/* copy one reference-layout vector to the host; `dir` = 0 fw / 1 bw for LSTM internals.   [sync] */
int  cn_layer_read(cn_layer *layer, cn_buffer which, int dir, float *host, size_t count);
/* overwrite a flat parameter vector (WEIGHTS / WEIGHT_UPDATES / WEIGHT_DELTAS) from the host: batch-mode
 * accumulation (Optimizer.cu:72-85) and optimizer-state restore (SteepestDescentOptimizer.cu:125-131) */
int  cn_layer_upload(cn_layer *layer, cn_buffer which, const float *host, size_t count);
/* overwrite Layer::outputErrors() from the host (tests of a single layer's backward pass) */
int  cn_layer_write_output_errors(cn_layer *layer, const float *host, size_t count);
/* raw fp32 device pointer of a flat parameter vector (WEIGHTS / WEIGHT_UPDATES / WEIGHT_DELTAS),
 * valid until the layer is destroyed; SteepestDescentOptimizer.cu:83-85 reads the same pointers */
void *cn_layer_device_ptr(cn_layer *layer, cn_buffer which);

/* All trainable layers of a context share one parameter arena [weights | weightUpdates | deltas];
 * the weightUpdates part is what the data-parallel all-reduce sums.  The arena is
 * laid out at the first call of this function / the first forward pass; creating a trainable layer
 * afterwards fails with CN_ERR_STATE. */
int  cn_ctx_param_arena(cn_ctx *ctx, void **weights, void **weight_updates, void **weight_deltas,
                        size_t *count);

/* Tell the library that the flat weights were modified through a raw device pointer (e.g. by an
 * external optimizer); the packed copies are rebuilt before the next forward pass. */
int  cn_ctx_weights_touched(cn_ctx *ctx);

/* UpdateWeightFn (SteepestDescentOptimizer.cu:39-59): delta = momentum*delta - lr*update;
 * w += delta; then refresh the packed device copies the kernels read. */
int  cn_sgd_update(cn_layer *layer, float learning_rate, float momentum);
/* per-layer learning rate (the JSON "learningRate" of TrainableLayer.cu:58; negative = none) that cn_sgd_update_all
 * uses for this layer instead of its argument, as SteepestDescentOptimizer.cu:78-80 does */
int  cn_layer_set_learning_rate(cn_layer *layer, float learning_rate);
/* the same update for every trainable layer of the context in one launch; layers with a learning rate of their own
 * (cn_layer_set_learning_rate) are updated with it */
int  cn_sgd_update_all(cn_ctx *ctx, float learning_rate, float momentum);
/* Arms the update of the COMING backward pass (the per-fraction protocol of Optimizer.cu:86-94, hybrid online/batch learning):
 * each layer applies UpdateWeightFn with these values -- or its own learning rate -- as soon as its own gradient is complete,
 * on the stream that computed it (behind its all-reduce when a communicator is bound), instead of for all layers behind the
 * last backward kernel.  The result is the one of cn_layer_backward on every layer followed by cn_sgd_update_all: a layer's
 * weights are last read by its own backward pass, so the layers below never see the difference; only a cn_layer_read of
 * CN_BUF_WEIGHTS between the two calls would.  The following cn_sgd_update_all(ctx, same values) -- or cn_sgd_update per
 * layer -- completes the step (waits, handles layers no backward call reached) and disarms; it is an error to start another
 * backward pass before it.  Not for batch learning (the epoch sum is formed first).  Weight noise generated on the device
 * (cn_ctx_set_weight_noise) goes with it; the reference's host protocol, which uploads noisy weights and restores them behind
 * the backward pass, does not.                                                                                    [async] */
int  cn_ctx_arm_update(cn_ctx *ctx, float learning_rate, float momentum);

/* Batch learning (`--stochastic false`): Optimizer.cu:72-85 sums the fractions' weightUpdates of an epoch on the DEVICE
 * (thrust::copy for the first fraction, thrust::transform(plus) for the others) and updates once per epoch (:95-97).
 * cn_ctx_accumulate_updates adds the weightUpdates of ALL layers, as the backward pass of the current fraction left them, to
 * the context's epoch accumulator in one launch (first != 0: copies instead, the reference's `firstFraction` branch);
 * cn_ctx_take_accumulated makes the epoch sum the weightUpdates of every layer again -- what SteepestDescentOptimizer.cu:83-85
 * reads through `_curWeightUpdates()` -- in front of cn_allreduce_grads(ctx, NULL, 0) / cn_sgd_update*.  Nothing leaves the
 * device and nothing synchronises.                                                                               [async] */
int  cn_ctx_accumulate_updates(cn_ctx *ctx, int first);
int  cn_ctx_take_accumulated(cn_ctx *ctx);

/* ---- data-parallel training over the GPUs of one node (no counterpart in the reference, which
 *      drives a single device: main.cpp:526-541) ------------------------------------------------------------
 * One process (or thread) per GPU, one cn_ctx each.  The parallel sequences of a fraction are independent, so
 * ranks take disjoint sequences and meet only in the SUM over patterns of the weight gradients
 * (LstmLayer.cu:502-510, FeedForwardLayer.cu:94-100,206) and in the scalar error / #correct: one all-reduce(SUM)
 * of weightUpdates per layer on RCCL over xGMI, then the identical UpdateWeightFn on every rank keeps the replicas
 * bit-identical without a broadcast.  librccl is opened at run time (dlopen "librccl.so.1"; a process that already
 * holds one, e.g. through PyTorch, shares it); the library has no link-time dependency on it. */
/* CN_COMM_BACKEND=p2p in the environment selects the library's NATIVE exchange in place of RCCL, behind the same entry points:
 * a shared-memory rendezvous named by the id, one region per rank (flag words + two staging halves) mapped into every peer
 * through hipIpc, and cn_allreduce_grads = ONE stream-ordered kernel per bucket that stages, signals, sums in rank order and
 * acknowledges through the peers' regions -- one shot for small buckets, reduce-scatter + all-gather over the full xGMI mesh
 * for large ones (csrc/cn_comm_p2p.hip, csrc/cn_comm_ipc.cpp).  No host barrier after the first bucket; a peer that does not
 * answer within CN_COMM_IPC_TIMEOUT seconds (default 120) fails the communicator and the next cn_loss_read_global raises
 * CN_ERR_COMM.  One node, at most 8 ranks.  RCCL stays the default. */
/* (Tests on a box with fewer GPUs than ranks: with CN_COMM_BACKEND=ipc in the environment the four entry points below keep their
 * contract on a host-blocking TEST backend for ranks that share a device -- a shared-memory rendezvous named by the id, hipIpc
 * staging buffers, sums in rank order (csrc/cn_comm_ipc.cpp).  Never a measurement.  The p2p backend runs with shared devices
 * too.) */
#define CN_COMM_ID_BYTES 128
/* rank 0: a fresh rendezvous id (ncclGetUniqueId); hand its 128 bytes to every rank out of band (pipe, file, MPI, ...) */
int  cn_comm_unique_id(char *id /* [CN_COMM_ID_BYTES] */);
/* collective over all `world` ranks: binds a communicator for ctx's device to the context (ncclCommInitRank) */
int  cn_comm_init(cn_ctx *ctx, const char *id /* [CN_COMM_ID_BYTES] */, int rank, int world);
int  cn_comm_destroy(cn_ctx *ctx);
/* rank / world size of the bound communicator; world = 0 when there is none.  Either pointer may be NULL. */
int  cn_comm_info(const cn_ctx *ctx, int *rank, int *world);
/* which exchange the bound communicator runs: "rccl", "p2p" or "ipc" ("" when there is none); *exchanges (may be NULL): the
 * number of all-reduces cn_allreduce_grads has enqueued on it so far */
const char *cn_comm_backend(const cn_ctx *ctx, int64_t *exchanges);
/* all-reduce(SUM, fp32, in place) of the weightUpdates of `n` layers, in the order given, on the context's
 * communication stream: that stream waits for each layer's gradient work only (not for what the context's stream has
 * enqueued since: the backward pass of the layers below keeps running beside the exchange), and the context's stream
 * waits for the reductions in front of the next cn_sgd_update* / cn_layer_read.  Call it right after
 * cn_layer_backward(layer) for "bucket = layer" overlap.  n == 0 (layers may be NULL): the whole weightUpdates arena
 * of the context in ONE all-reduce, after all gradient work.  Collective: every rank makes the same calls in the same
 * order.                                                                                              [async] */
int  cn_allreduce_grads(cn_ctx *ctx, cn_layer *const *layers, int n);
/* cn_loss_read over all ranks: all-reduce(SUM) of the device-side error / #correct sums, then read.   [sync] */
int  cn_loss_read_global(cn_ctx *ctx, float *error_sum, int64_t *correct_sum, int reset);

/* ---- measurement ---------------------------------------------------------------------------- */

/* Wrap hipEvents around the kernels of one class on the ctx stream and accumulate their device
 * time; used by bench.py for the live roofline figure.  kernel_class: 0 = recurrent forward,
 * 1 = recurrent backward, 2 = N-wide gate GEMMs, 3 = weight-gradient GEMMs, 4 = everything else,
 * 5 = the gradient all-reduces of cn_allreduce_grads (events on the communication stream). */
int  cn_ctx_timing_enable(cn_ctx *ctx, int enable);
int  cn_ctx_timing_read(cn_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches); /* [sync] */
int  cn_ctx_timing_reset(cn_ctx *ctx);
/* name of the recurrent kernel the layer's last forward (backward != 0: backward) pass launched, recorded by the launcher
 * that instantiated it, e.g. "lstm_bwd_s2_kernel<0,128>", "lstm_fwd_kernel<2,128,1,1>" or
 * "lstm_bwd_cluster_kernel<0,256,128,1>"; "" for other layers and before the first pass */
const char *cn_layer_recurrent_kernel(cn_layer *layer, int backward);

/* ---- Weight averaging (no counterpart in the reference; Polyak & Juditsky 1992, the exponential form of Tarvainen & Valpola
 *      2017) ------------------------------------------------------------------------------------------------------------------
 * An exponential moving average of the weights beside the weights themselves, and the exchange of the two: a validation pass, a
 * stopping decision and an exported network may then use the smoothed model while training goes on with the raw one.
 *
 * State.  avg is ONE fp32 vector the length of the parameter arena (`count` of cn_ctx_param_arena, arena order, pad entries
 * included), an allocation of its own made by the first call that needs it.  The library keeps no clock (as with Adam's `step`):
 * the caller gives the decay of each step.
 *
 * The step, per arena entry, from the float argument `decay` in [0, 1):
 *      omd = (float)(1.0 - (double)decay)                                    rounded once
 *      avg = (omd == 1.0f) ? w : add_rn(avg, mul_rn(omd, sub_rn(w, avg)))
 * Every *_rn is a single fp32 operation rounded to nearest, no contraction, denormals kept, as for Adam.  omd == 1 is an exact copy
 * (avg + (w - avg) is not w in fp32: avg = 1, w = 1e-10).  The FIRST step of a context -- no average exists yet and none was
 * uploaded -- copies, whatever the decay.  The step does not look at the clipping record: behind a skipped update it moves avg
 * towards the unchanged w.  Data-parallel: every rank averages the same weights, so the replicas stay bit-identical without an
 * exchange.
 *
 * The swap exchanges w and avg entry by entry over the arena and toggles the context's "swapped" flag; every trainable layer's
 * operand copies become stale (what cn_ctx_weights_touched does), the noisy sets too.  The next forward pass reads the average; a
 * second swap restores every bit.  While swapped, cn_layer_read(CN_BUF_WEIGHTS) returns the average and
 * cn_layer_read_weight_average the raw weights; forward passes, loads, loss calls and reads stay allowed, and everything that
 * would train on, update or overwrite the exchanged weights fails with CN_ERR_STATE: cn_layer_backward, cn_sgd_update*,
 * cn_adam_update*, cn_ctx_arm_update, cn_ctx_arm_adam, cn_ctx_accumulate_updates, cn_ctx_take_accumulated, cn_allreduce_grads,
 * cn_ctx_average_weights, cn_layer_set_weights, cn_layer_upload, cn_layer_upload_weight_average.
 *
 * Without any of these calls the library launches exactly what it launches without them and allocates nothing for them. */
/* One averaging step over the whole arena with this decay, behind everything that wrote the weights.  A decay that is negative,
 * >= 1 or NaN: CN_ERR_BAD_ARG.                                                                                        [async] */
int  cn_ctx_average_weights(cn_ctx *ctx, float decay);
/* Exchanges the weights and their average.  Without an average, or while an armed update is pending (cn_ctx_arm_update /
 * cn_ctx_arm_adam not yet completed by the *_update* call): CN_ERR_STATE.                                              [async] */
int  cn_ctx_swap_weight_average(cn_ctx *ctx);
/* *exists: an average has been formed or uploaded; *swapped: the weights and the average are exchanged right now.  Either pointer
 * may be NULL. */
int  cn_ctx_weight_average_state(const cn_ctx *ctx, int *exists, int *swapped);
/* The layer's part of the average, flat reference layout like CN_BUF_WEIGHTS; before an average exists: the weights (what the
 * first step will copy).  A layer without weights: CN_ERR_BAD_ARG; count != cn_layer_weight_count: CN_ERR_SHAPE.       [sync] */
int  cn_layer_read_weight_average(cn_layer *layer, float *host, size_t count);
/* Overwrites the layer's part of the average from the host (autosave / --continue).  Creates the average if there is none: it
 * starts as a copy of ALL weights, then this layer's part is overwritten; the averaging step that follows does not copy.  Errors
 * as for the read. */
int  cn_layer_upload_weight_average(cn_layer *layer, const float *host, size_t count);

/* ---- Adam (no counterpart in the reference, whose option table names steepest_descent and rprop only,
 *      Configuration.cpp:152,265) ---------------------------------------------------------------------------------
 * A second update rule beside UpdateWeightFn, with the same three entry points and the same protocol as the cn_sgd_* trio.
 *
 * Arithmetic.  All state is fp32.  g is the layer's weightUpdates entry, the quantity the steepest-descent step reads.  The
 * first moments m live in the weightDeltas part of the parameter arena (CN_BUF_WEIGHT_DELTAS; cn_ctx_param_arena is unchanged),
 * the second moments v in one more vector of the same length (CN_BUF_ADAM_SECOND_MOMENTS), zero at the first Adam call unless
 * uploaded.  The library keeps no clock: `step` (>= 1) is the caller's count of updates, this one included.  From the float
 * arguments the host forms, in double, rounded once to float,
 *      omb1 = 1 - beta1      omb2 = 1 - beta2
 *      alpha_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step)        (product first, then the quotient)
 *      eps_t   = eps * sqrt(1 - beta2^step)
 * and the device computes per weight, every operation an fp32 operation rounded to nearest on its own (no contraction, correctly
 * rounded square root and division, denormals kept):
 *      m = beta1*m + omb1*g
 *      v = beta2*v + omb2*(g*g)
 *      w = w - (alpha_t*m) / (sqrt(v) + eps_t)
 * which is algebraically Adam with bias correction (Kingma & Ba 2015; torch.optim.Adam without amsgrad and weight decay).  Every
 * path -- the flat kernel, and the forms fused into the operand-copy launch -- computes exactly this, bit for bit.
 *
 * Binding.  weightDeltas is the momentum term under steepest descent and the first moment under Adam, so a context belongs to the
 * family of its first update or arm call; a later call of the other family fails with CN_ERR_STATE.  step < 1, a beta outside
 * [0, 1) and eps <= 0 fail with CN_ERR_BAD_ARG. */
/* beside cn_sgd_update (UpdateWeightFn, SteepestDescentOptimizer.cu:39-59; the reference has no counterpart): the Adam step of
 * one layer with `learning_rate` as given, then the packed copies are refreshed before the next forward pass */
int  cn_adam_update(cn_layer *layer, float learning_rate, float beta1, float beta2, float eps, int64_t step);
/* beside cn_sgd_update_all (SteepestDescentOptimizer::_updateWeights, SteepestDescentOptimizer.cu:67-94; the reference has no
 * counterpart): every trainable layer in one launch, operand copies included; a layer with a learning rate of its own
 * (cn_layer_set_learning_rate) takes it as its lr.  Orders itself behind cn_allreduce_grads like cn_sgd_update_all. */
int  cn_adam_update_all(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step);
/* beside cn_ctx_arm_update (the per-fraction protocol of Optimizer.cu:86-94 around SteepestDescentOptimizer.cu:67-94; the
 * reference has no counterpart): arms the Adam step of the COMING backward pass, applied per layer as soon as its gradient is
 * complete.  Completed by cn_adam_update_all(ctx, same values) or by cn_adam_update per layer (same values; a layer with a
 * learning rate of its own passes that), else CN_ERR_STATE; cn_ctx_accumulate_updates is refused while it is armed.   [async] */
int  cn_ctx_arm_adam(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step);

/* ---- Dropout on the connections between layers (no counterpart in the reference; Pham et al. 2014, Zaremba et al. 2014) -------
 * Dropout belongs to a trainable layer and acts on that layer's INPUT, the connections from the preceding layer: the layer's input
 * products (forward, and the input-weight gradient) read a masked, rescaled copy of the preceding layer's outputs, and the error
 * handed back to the preceding layer passes the same mask.  The preceding layer's own outputs, its recurrence and CN_BUF_OUTPUTS
 * are untouched; nothing inside a time loop drops.
 *
 * The mask.  rate in [0, 1).  n = t*PS + ps is the frame in the reference layout (PS = parallel_sequences as given to the input
 * layer), i the unit of the preceding layer in the reference layout, 0 <= i < P (blstm: the forward units, then the backward ones).
 *      (w0,w1,w2,w3) = Philox4x32-10( counter = (i >> 2, n, pass_lo, pass_hi),
 *                                     key     = ((seed_lo + ordinal) mod 2^32, seed_hi) )
 *      keep(n,i)     = w[i & 3] >= thr        thr   = (uint32) floor((double)rate * 2^32)
 *      x'(n,i)       = keep ? x(n,i) * scale : 0        scale = (float)(1.0 / (1.0 - (double)rate))
 * (Philox4x32-10 of Salmon et al. 2011: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten rounds; counter
 * and key words in the order written, _lo / _hi the halves of the 64-bit values.)  `ordinal` is the index of the dropping layer in
 * the context's creation order, the input layer being 0.  `seed` and `pass` are the caller's: the library keeps no clock, as with
 * Adam's `step`.  The product is ONE fp32 multiplication, then rounded to the operand type (CN_PREC_BF16: to nearest even;
 * CN_PREC_F32 / CN_PREC_BF16X3: kept as fp32).  Backward: e'(n,i) = keep ? e(n,i) * scale : 0, one fp32 multiplication, the same
 * mask.  The mask is a function of (seed, pass, ordinal, n, i, rate) alone: not of any padding, the precision mode or the kernels
 * chosen.
 *
 * With dropout disabled, or every rate 0, the library launches exactly what it launches without these calls and allocates
 * nothing for them. */
/* The JSON "dropout" of a layer.  lstm, blstm, feedforward_* and softmax layers; any other kind, and a rate outside [0, 1):
 * CN_ERR_BAD_ARG.  May be called between fractions.  The first non-zero rate allocates the layer's masked operand copy (the size
 * of the preceding layer's operand copy); rate 0 takes the layer off the dropout path again. */
int  cn_layer_set_dropout(cn_layer *layer, float rate);
/* Whether the forward passes that follow drop (enable != 0), and with which (seed, pass), until the next call; a fresh context
 * does not.  Each layer records in its forward pass whether it dropped and with which key, rate included, and its backward pass
 * uses that record: a call between forward and backward cannot tear a step. */
int  cn_ctx_set_dropout_pass(cn_ctx *ctx, int enable, uint64_t seed, uint64_t pass);

/* ---- Gradient clipping by the global L2 norm (Pascanu et al. 2013; no counterpart in the reference, whose only guard is the
 *      per-element delta clip inside the LSTM cell, which the kernels keep) ------------------------------------------------------
 * One bound on the size of a step, in front of the momentum rule and the Adam rule alike.
 *
 * The gradient.  g is the weightUpdates part of the parameter arena: all n = `count` entries of cn_ctx_param_arena in arena order
 * (every layer's flat vector, each rounded up to a multiple of four entries by pad entries that are zero), as the update is about
 * to read it: after cn_allreduce_grads, and after cn_ctx_take_accumulated (batch learning clips the epoch sum).
 *
 * The sum.  S = sum of g[i]^2 is formed in DOUBLE; each square is formed in double from the float, so it is exact.  The order
 * is a function of i and n alone -- not of the grid, the CU count, the precision mode or the "deterministic" option:
 *      L = 16384 lanes.  lane[k] = ((0 + g[k]^2) + g[k + L]^2) + g[k + 2L]^2 + ...   ascending, entries i >= n count as +0
 *      then fourteen levels over NEIGHBOURING lanes:  lane'[k] = lane[2k] + lane[2k + 1]  (L/2 sums, then L/4, ... then one) = S
 * (numpy: pad g to a multiple of L, acc = zeros(L, float64); for each row r of g.reshape(-1, L): acc += r.astype(float64) ** 2;
 * while len(acc) > 1: acc = acc[0::2] + acc[1::2].)
 *
 * The norm and the factor.  norm = (float) sqrt(S): a correctly rounded double square root, rounded once to float.
 *      S not finite (an inf or NaN entry):  the step is SKIPPED
 *      else norm > max_norm:                scale = max_norm / norm, one correctly rounded fp32 division, and every path uses
 *                                           g' = scale * g (one fp32 multiplication) in place of g
 *      else:                                no multiplication happens at all: a step whose norm stays at or below the bound is
 *                                           bit-equal to the same step with clipping off
 * A skipped step leaves the weights, the deltas / first moments, the second moments and the operand copies as they were, bit for
 * bit.  The caller's Adam `step` still advances: the library keeps no clock.  weightUpdates itself is never rewritten:
 * cn_layer_read(CN_BUF_WEIGHT_UPDATES) after the update returns the unclipped gradient.  Per-layer learning rates keep their
 * meaning: the factor is global, the rates are per layer.
 *
 * When.  The norm is formed once per gradient, on the context's stream, by the first cn_sgd_update / cn_sgd_update_all /
 * cn_adam_update / cn_adam_update_all after the gradient last changed (cn_layer_backward, cn_allreduce_grads,
 * cn_ctx_take_accumulated, cn_layer_upload of CN_BUF_WEIGHT_UPDATES); later per-layer calls of the same step reuse it.  Nothing
 * synchronises the host.  Data-parallel: every rank forms the norm of the same reduced gradient in the same order, so the replicas
 * stay bit-identical without another exchange.
 *
 * Armed updates.  A global norm needs every layer's gradient, so the step cannot be applied layer by layer behind each gradient.
 * With clipping on, cn_ctx_arm_update / cn_ctx_arm_adam are still accepted and checked, and the step is applied by the completing
 * *_update* call (which must name the armed values, else CN_ERR_STATE); the caller's call sequence and the result -- backward on
 * every layer, then *_update_all -- are unchanged, the overlap of the update with the backward pass is lost.
 *
 * With clipping off the library launches exactly what it launches without these calls and allocates nothing for them. */
/* The bound; 0 = off, and a fresh context is off.  Negative, NaN or infinite: CN_ERR_BAD_ARG.  May be changed between steps; while an
 * armed update is pending: CN_ERR_STATE.  max_norm = FLT_MAX makes a pure monitor: the norm is formed, nothing is ever scaled. */
int  cn_ctx_set_grad_clip(cn_ctx *ctx, float max_norm);
/* The record of the last step whose norm was formed -- *last_norm, *last_scale (the factor; 1 when the step was not clipped, 0 when
 * it was skipped) -- and, since the last reset: the norms formed (*updates), the steps clipped and skipped, and the largest finite
 * norm.  Any pointer may be NULL; reset != 0 clears the counters and the largest norm behind the read.  With clipping off it
 * reports zeros.                                                                                                      [sync] */
int  cn_ctx_grad_clip_stats(cn_ctx *ctx, float *last_norm, float *last_scale, int64_t *updates, int64_t *clipped, int64_t *skipped,
                            float *max_norm_seen, int reset);

/* ---- Weight decay (decoupled: Loshchilov & Hutter 2019, "Decoupled Weight Decay Regularization"; no counterpart in the
 *      reference) -----------------------------------------------------------------------------------------------------------------
 * One rule, in front of the momentum rule and of the Adam rule alike: the weight shrinks by a fraction of itself that does not pass
 * through the gradient, the momentum term or Adam's moments.  (Not the coupled L2 term g + decay * w.)
 *
 * The rule.  decay is a setting of the context, a float >= 0.  Per update of a layer the host forms
 *      ld = (float)((double) lr_layer * (double) decay)                      rounded once
 * where lr_layer is the rate that layer's step uses: the call's learning rate, or the layer's own (cn_layer_set_learning_rate).
 * Under Adam ld uses the learning rate, not alpha_t.  Per weight the device computes
 *      w0 = sub_rn(w, mul_rn(ld, w))                                         two fp32 operations, each rounded to nearest, no
 *                                                                            contraction, denormals kept
 * and the family's step runs with w0 in place of w:
 *      momentum:  dl = mom * dl - lr * g;  w = add_rn(w0, dl)
 *      Adam:      w = sub_rn(w0, (alpha_t * m) / (sqrt(v) + eps_t))          exactly as cn_adam_update states it
 * The LAMB family (section LAMB) does NOT apply this rule: there the term decay * w of the same weights enters the direction u, in
 * front of the layer's trust ratio, and no w0 is formed.
 *
 * What decays.  Input weights and internal (recurrent) weights only.  Bias weights, peephole weights and the arena's pad entries
 * never do: for them w0 = w and no operation is performed.  In the flat reference layout of a layer with L units, P inputs and
 * H = L / directions:
 *      lstm / blstm:              [0, 4LP) and [4L(P+1), 4L(P+1) + 4LH) decay; the bias block [4LP, 4L(P+1)) and the trailing 3L
 *                                 peephole weights do not
 *      feedforward_* / softmax:   [0, LP) decays, the trailing L bias weights do not
 *
 * Order and interactions.  The clipping factor scales g only, and the decay term is no part of the norm.  A step the clipping
 * record skips decays nothing: weights, deltas / moments and operand copies keep every bit.  Batch learning decays once per
 * update, not per fraction.  Weight noise and weight averaging see the decayed weights as the weights.  Data-parallel: every rank
 * decays the same weights by the same ld, so the replicas stay bit-identical without an exchange.  Armed updates stay overlapped
 * with the backward pass (decay is local to a weight) unless clipping defers them; an armed step uses the decay in force when it
 * was armed.  The operand copies a fused or armed step writes hold the decayed, updated weight.
 *
 * With decay 0 the library launches exactly what it launches without these calls and allocates nothing for them. */
/* The coefficient; 0 = off, and a fresh context is off.  Negative, NaN or infinite: CN_ERR_BAD_ARG.  May be changed between steps;
 * while an armed update is pending (armed or deferred): CN_ERR_STATE.  Allowed while the weights are swapped with their average:
 * it only stores a number. */
int  cn_ctx_set_weight_decay(cn_ctx *ctx, float decay);
int  cn_ctx_get_weight_decay(const cn_ctx *ctx, float *decay);

/* ---- Weight noise (--weight_noise_sigma, Optimizer.cu:58-84: the reference's only regulariser) ----------------------------------
 * Gaussian noise on the weights, seen by the backward pass alone: every backward product with a weight in it reads w' = w + n, while
 * the forward pass, the error and the update see the clean weights.  The reference draws the noise on the host; here it is
 * generated on the device, straight into a second set of the operand copies a backward pass reads (an LSTM layer's transposed
 * input weights, transposed recurrent weights and peephole weights; a dense layer's transposed weights).  The bias weights are
 * read by no backward pass.  CN_BUF_WEIGHTS, the parameter arena and the copies a forward pass reads never hold noise: nothing
 * needs restoring, and a forward pass behind a noisy backward pass without an update is bit-equal to one with noise off.
 *
 * The noise.  For a trainable layer with creation ordinal `ordinal` (as for dropout) and flat weight index k in the reference
 * layout, 0 <= k < cn_layer_weight_count:
 *      (w0,w1,w2,w3) = Philox4x32-10( counter = (k >> 2, 0, pass_lo, pass_hi),
 *                                     key     = ((seed_lo + ordinal) mod 2^32, seed_hi XOR 0x6E6F6973) )
 *      pair p = (k & 3) >> 1 uses words (w[2p], w[2p+1]) = (a, b)
 *      u1 = (float)(2*(a >> 9) + 1) * 2^-24        in (0,1), exact in fp32
 *      t  = (float)(2*(b >> 9) + 1) * 2^-23        in (0,2), exact in fp32   (= 2*u2)
 *      r  = sqrt_rn( mul_rn(-2, logf(u1)) )
 *      z  = mul_rn(r, (k & 1) ? sinpif(t) : cospif(t))        Box-Muller, both outputs of a pair used
 *      n  = mul_rn(sigma, z)
 *      w' = add_rn(w, n)                                      then rounded ONCE to the operand type (CN_PREC_BF16: to nearest even)
 * Every *_rn is a single fp32 operation rounded to nearest, no contraction; the square root is correctly rounded; logf, sinpif and
 * cospif are the device library's.  The key's XOR constant ("nois") keeps the stream apart from the dropout masks of the same
 * seed.  The noise is a function of (seed, pass, ordinal, k, sigma) alone: not of any padding, the precision mode, the kernels
 * chosen or the rank.  Padding entries of the noisy copies are exactly zero.
 *
 * Works with both update rules, armed updates (the fused per-layer update runs behind a noisy backward pass: it rebuilds the
 * clean copies only), clipping, dropout, the deterministic mode, batch learning and a bound communicator, in all three precisions.
 * With noise off the library launches exactly what it launches without this call and allocates nothing for it. */
/* sigma == 0: off, and a fresh context is off.  Negative, NaN or infinite: CN_ERR_BAD_ARG.  `seed` and `pass` are the caller's (the
 * library keeps no clock).  Each layer's cn_layer_backward uses the triple in force when it is called.  The first non-zero sigma
 * that reaches a backward pass allocates the noisy copies.                                                        [async] */
int  cn_ctx_set_weight_noise(cn_ctx *ctx, float sigma, uint64_t seed, uint64_t pass);

/* ---- Input augmentation (--input_noise_sigma, DataSet.cpp:177-184: drawn there on the loader thread; SpecAugment's frequency and
 *      time masks, Park et al. 2019: no counterpart in the reference) -------------------------------------------------------------
 * Gaussian noise on the input patterns and masks over runs of features and of frames, applied on the device where a fraction is
 * re-laid out: the augmented inputs ARE the input layer's outputs.  cn_layer_read(input, CN_BUF_OUTPUTS) returns them, the first
 * layer's forward product and input-weight gradient read them, nothing keeps the clean ones.  Targets, classes, pattern types
 * and the row map are untouched.
 *
 * Geometry.  P is the input layer's size, B = context_left + context_right + 1 the frames the caller spliced into one pattern,
 * P0 = P / B the features of a frame; P % B != 0 makes the load fail with CN_ERR_SHAPE.  For slot s (0 <= s < PS), time t and
 * column c of the pattern:
 *      block b = c / P0        feature j = c % P0        source frame ts = clamp(t + b - context_left, 0, len_s - 1)
 * len_s is the number of frames of slot s whose pattern type is not NONE (a sequence lies in its slot from t = 0 without holes).  A
 * frame whose pattern type is NONE is copied unchanged, and so is everything in a slot with len_s = 0.  Noise and masks are
 * functions of the SOURCE element (s, ts, j): every context copy of a frame carries the same noise and the same masks, which is
 * what adding the noise before splicing gives (DataSet.cpp:177-190).
 *
 * The noise.  e = ts*P0 + j,
 *      (w0,w1,w2,w3) = Philox4x32-10( counter = (e >> 2, s, pass_lo, pass_hi),
 *                                     key     = (seed_lo, seed_hi XOR 0x696E7074) )
 * and from there exactly the formulas of section Weight noise with e in the place of k: pair (e & 3) >> 1, u1, t, r,
 * z = mul_rn(r, (e & 1) ? sinpif(t) : cospif(t)), n = mul_rn(sigma, z), x' = add_rn(x, n): every step a single fp32 operation.
 * The constant ("inpt") keeps the stream apart from the weight noise and the dropout masks of the same seed.  With
 * noise_sigma == 0 nothing is added (x' = x, bit for bit).
 *
 * The masks.  For each slot with len_s >= 1, mask m draws
 *      (w0,w1,.,.) = Philox4x32-10( counter = (m, s, pass_lo, pass_hi), key = (seed_lo, seed_hi XOR 0x6D61736B) )       ("mask")
 * Frequency mask i uses m = i, time mask i uses m = 16 + i: a mask does not depend on how many of the other kind there are.
 *      frequency mask:  Fc = min(freq_width, P0)                                      w = w0 mod (Fc + 1)
 *                       f0 = w1 mod (P0 - w + 1)                                      covers features     f0 <= j  < f0 + w
 *      time mask:       Wc = min(time_width, len_s * time_max_permille / 1000)        w = w0 mod (Wc + 1)       (integer division)
 *                       t0 = w1 mod (len_s - w + 1)                                   covers source frames t0 <= ts < t0 + w
 * A covered element becomes exactly +0.0, noise or not: the mean of standardised features.  (The bias of the modulo, at most
 * 2^-32 * range, is ignored.)
 *
 * The result is rounded ONCE to the operand type (CN_PREC_BF16: to nearest even; fp32 otherwise) and is a function of
 * (settings, s, ts, j, x) alone: not of any padding, the precision mode, the load path or the kernels chosen.  Pad slots and pad
 * columns stay exactly zero.
 *
 * When.  Every cn_fraction_load and cn_fraction_load_resident re-lays the fraction out with the settings in force when it is
 * called, on every path (resident, staged host upload, the strided copies of option overlap = 0).  cn_fraction_prefetch* records
 * the settings in force at the prefetch; the load that follows is a hit only if the settings in force at the load equal the
 * recorded ones member by member -- otherwise the prefetch is discarded like any other miss and the load runs the ordinary way.
 * What a load leaves behind is therefore always a function of the settings at the load.
 *
 * With a == NULL, or noise_sigma == 0 and both counts 0, the library launches exactly what it launches without the call. */
typedef struct cn_input_augment {
    float    noise_sigma;                  /* >= 0, finite; 0 = no noise                                   */
    int      context_left, context_right;  /* how the caller spliced the patterns it loads (>= 0)          */
    int      freq_masks, freq_width;       /* number of frequency masks (0..8), largest width F (>= 0)     */
    int      time_masks, time_width;       /* number of time masks (0..8), largest width W (>= 0)          */
    int      time_max_permille;            /* 0..1000: a time mask is at most len * this / 1000 frames     */
    uint64_t seed, pass;                   /* the caller's: the library keeps no clock                     */
} cn_input_augment;
/* NULL = off, and a fresh context is off.  CN_ERR_BAD_ARG: a negative, NaN or infinite noise_sigma; a negative context, width or
 * count; a count above 8; time_max_permille outside 0..1000.  (P % B != 0 is found at the load: CN_ERR_SHAPE.)  The first enabling
 * call allocates the per-slot mask table (a few hundred bytes per slot; a second one with the first prefetch); turning the
 * augmentation off again leaves them unused until the context is destroyed.                                      [async] */
int  cn_ctx_set_input_augment(cn_ctx *ctx, const cn_input_augment *a);

/* ---- Input splicing and frame skipping (--input_left_context / --input_right_context, DataSet.cpp:346-366: spliced there on the
 *      host; the frame skip, "low frame rate" input, has no counterpart in the reference) ------------------------------------------
 * With the setting on, every cn_fraction_load, cn_fraction_load_resident, cn_fraction_prefetch and cn_fraction_prefetch_resident
 * that follows takes its cn_fraction at SOURCE rate, unspliced, and the library derives the network-rate fraction on the device,
 * where it re-lays the fraction out: the upload carries every frame once, and every layer runs on every K-th frame only.
 *
 * Let L, R, K be the three members, B = L + R + 1, P the input layer's size and P0 = P / B.  The source fraction:
 *      max_seq_length = Tsrc, min_seq_length = Tmin_src; pat_types, target_classes and targets have Tsrc * PS rows; inputs is
 *      [Tsrc * PS][P0]; input_pattern_size = P0.
 * P % B != 0, input_pattern_size != P0 and ceil(Tsrc / K) above the layers' max_seq_length each fail the load with CN_ERR_SHAPE.
 *
 * The network-rate fraction, which is all that every later layer sees:
 *      len_s = frames of slot s whose pattern type is not NONE (a sequence lies in its slot from t = 0 without holes)
 *      n_s = ceil(len_s / K)        T' = ceil(Tsrc / K)        Tmin' = ceil(Tmin_src / K)
 * Network frame (j, s) with j < n_s:
 *      pattern type   FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL otherwise: those of a sequence of n_s frames
 *      input column c block b = c / P0, feature f = c % P0, source frame ts = clamp(K*j + b - L, 0, len_s - 1):
 *                     inputs[(ts*PS + s)*P0 + f], rounded ONCE to the operand type
 *      target class and target row: those of source row K*j, the frame the context is centred on.  (A lag of the targets is the
 *                     caller's, applied at source rate before the load.)
 * j >= n_s, pad slots and pad columns: NONE, zeros, class -1, zero targets, as without the setting.  The row map is built from
 * the derived pattern types, with Tmin' time steps of unchecked rows.  The current fraction has T' and Tmin' steps: cn_layer_read
 * of any layer returns T' * PS rows.  A CTC layer is unaffected: cn_layer_set_label_sequences brings the labels, and
 * num_sequences is the caller's.  With K = 1 this is bit for bit what a load of the host-spliced fraction leaves.
 *
 * Together with cn_ctx_set_input_augment: the augmentation's context_left / context_right must equal L and R, otherwise the load
 * fails with CN_ERR_SHAPE.  Noise and masks stay the functions of the source element (s, ts, f) stated there, with ts as above;
 * len_s and the time masks count source frames.  With K = 1 the result is bit for bit that of a host-spliced load with the same
 * augmentation; with K > 1 it is the augmentation of the source fraction, then the gather.
 *
 * cn_fraction_prefetch* records the setting in force at the prefetch; the load that follows is a hit only if the setting in force
 * at the load equals it member by member.  With option overlap = 0 a host fraction is packed and uploaded like the staged route and
 * re-laid out by the same kernel; the call then waits for it.  The staging areas are sized by what a fraction needs under the
 * setting in force when they are allocated: a later setting whose fractions need more (a larger K, wider patterns) makes the next
 * host load or prefetch reallocate them, which synchronises the device once.
 *
 * The augmentation's rule needs the source frames.  A caller that skips frames on the host (a network-rate fraction, setting off)
 * and names a context to cn_ctx_set_input_augment gets the rule applied to the rows it loaded, as if they were consecutive frames:
 * with a skip above 1 augment through this setting instead.
 *
 * {0, 0, 1} is ON: the identity gather, which leaves what the plain load leaves.  With s == NULL, or without the call, the library
 * launches exactly what it launches today. */
typedef struct cn_input_splice { int context_left, context_right, frame_skip; } cn_input_splice;
/* NULL = off, and a fresh context is off.  CN_ERR_BAD_ARG: a negative context, a context above 32 per side, frame_skip outside
 * 1..16.  The first spliced load allocates the per-slot length table if the augmentation has not.                  [async] */
int  cn_ctx_set_input_splice(cn_ctx *ctx, const cn_input_splice *s);

/* ---- Residual connections (no counterpart in the reference; He et al. 2016, and Kim et al. 2017 for stacked LSTMs) ----------------
 * A hidden layer l of kind lstm, blstm or feedforward_{tanh,logistic,identity} whose preceding layer has the same `size` may be
 * marked residual; the preceding layer may be of any kind, the input layer included.  Write b for what l computes without the
 * mark, its "branch": l's operand copy, which its own recurrence and its recurrent-weight gradient keep reading.  What l's
 * followers and cn_layer_read(.., CN_BUF_OUTPUTS, ..) see for a real frame n and unit u is
 *      out[n][u] = round_op( float(b_op[n][u]) + float(x_op[n][u]) )
 * b_op: l's operand copy; x_op: what the preceding layer's followers read -- its own sum if it is residual too, never a dropped
 * copy; round_op: ONE rounding to the operand type (CN_PREC_F32 / CN_PREC_BF16X3: none, the fp32 sum; CN_PREC_BF16: to nearest
 * even).  Units are matched in the reference layout, unit u of both layers (blstm: the forward units, then the backward ones),
 * whatever padding either layer's rows have.  On rows that are not real frames (dummy frames, pad slots) out is the branch: 0
 * for an LSTM layer.  Pad columns of out are zeros.
 *
 * Backward.  l's outputErrors e, as its follower wrote them, are dL/d out.  The branch's backward pass uses e as it does without
 * the mark (a feed-forward layer's act' is taken at the branch output).  When the preceding layer is trainable its outputErrors
 * become (what l's backward pass hands back today, after the dropout mask if l drops) + e on real frames, unit by unit, one fp32
 * addition; dummy rows get nothing added.  Dropout on l's input acts on the weighted path only: the skip path is never dropped and
 * never rescaled.  Weight noise does not touch it.  This is part of the model, not a regulariser: every forward pass sums.
 *
 * With no layer marked the library launches exactly what it launches without this call and allocates nothing for it. */
/* The JSON "residual" of a layer.  CN_ERR_BAD_ARG: a layer of another kind; a size that differs from the preceding layer's; a
 * post output layer directly behind the layer (cn_layer_create of a post output layer behind a residual layer is refused as
 * well: the post output kernels read the fp32 outputs, and that case is left out).  May be called between fractions; takes effect
 * with the layer's next forward pass, and each layer's backward pass goes by what its forward pass did.  The first enabling call
 * allocates the layer's sum buffer (the size of its operand copy; a feed-forward layer: also an fp32 copy of its outputErrors). */
int  cn_layer_set_residual(cn_layer *layer, int enable);

/* ---- Layer normalization (no counterpart in the reference; Ba et al. 2016, "pre-LN": in front of the weighted path) ---------------
 * A trainable layer l (lstm, blstm, feedforward_*, softmax) may be marked: its input products then read a normalised copy of what
 * its preceding layer's followers read.  The preceding layer may be of any kind, the input layer included; its size P must be >= 2.
 *
 * The rule.  For a real frame n (pattern type not NONE, slot < PS), with x_i, i = 0..P-1, the operand values the preceding
 * layer's followers read for that frame (its sum if it is residual, never a dropped copy), taken as floats:
 *      mean = (1/P) sum_i x_i          var = (1/P) sum_i (x_i - mean)^2        two passes over the row, both sums formed in double
 *      rstd = 1 / sqrt(var + eps)      in double; mean and rstd each rounded once to float: mean_f, rstd_f
 *      xn_i = round_op( mul_rn( sub_rn(x_i, mean_f), rstd_f ) )
 * Every *_rn is a single fp32 operation rounded to nearest, no contraction; round_op: ONE rounding to the operand type
 * (CN_PREC_F32 / CN_PREC_BF16X3: none; CN_PREC_BF16: to nearest even); eps is the layer's, default 1e-5.  The order in which the
 * double sums are formed is the kernel's own: the result is held to a bound, not to bits, and is the same bits from run to run.
 * Units are the reference layout's: pad columns take no part in a statistic and are written as zeros.  Rows that are not real
 * frames (dummy frames, pad slots) are written as zeros, which keeps the row map's condition that every operand row of a dummy
 * frame is zero.
 *
 * There is no learned gain and no bias: xn is read only by l's own input products, and
 *      W (gamma * xn + beta) + b = (W diag gamma) xn + (W beta + b),
 * so a gain is absorbed by the columns of the input weights and a bias by the layer's bias weights (for an LSTM layer for all
 * four gates at once).  Nothing is added to the weights, the optimizers, the clipping norm or the all-reduce, and nothing is
 * summed over frames.
 *
 * Forward.  l's input products (and the input-weight gradient) read xn.  If l also drops, the dropout mask is applied to xn: the
 * order is normalisation, then dropout.  The preceding layer's own outputs, CN_BUF_OUTPUTS and a residual skip path never see the
 * normalisation: a residual l adds its un-normalised input.  This is part of the model, not a regulariser: every forward pass
 * normalises.
 *
 * Backward.  When the preceding layer is trainable, what l's backward pass hands back (after the dropout mask if l drops), g =
 * dL/d xn, is rewritten in place, in front of a residual l's skip term, as
 *      dx_i = rstd_f * ( g_i - mean(g) - xn_i * mean(g * xn) )        on real frames;  0 on every other row
 * with xn as the forward pass stored it (after round_op), rstd_f as the forward pass stored it, and both means formed in double over
 * the P units and rounded once to float.  Each layer's backward pass goes by what its forward pass did.
 *
 * With no layer marked the library launches exactly what it launches without this call and allocates nothing for it. */
/* The JSON "layer_norm" / "layer_norm_eps" of a layer.  CN_ERR_BAD_ARG: a layer that is not trainable; a preceding layer of size 1;
 * eps not finite or <= 0.  May be called between fractions; takes effect with the layer's next forward pass.  The first enabling
 * call allocates the normalised copy (the size of the preceding layer's operand copy) and one float per row. */
int  cn_layer_set_layer_norm(cn_layer *layer, int enable, float eps);

/* ---- Context layers (no counterpart in the reference, whose only splicing is that of the input patterns, DataSet.cpp:346-366;
 *      Waibel et al. 1989, Peddinti et al. 2015: time-delay layers) ----------------------------------------------------------------
 * A layer of its own kind, CN_LAYER_CONTEXT, without weights: its output for a frame is the preceding layer's output for that
 * frame and for its neighbours, side by side.  A feedforward_* layer behind it is a time-delay layer.  The preceding layer may be
 * of any kind that may have a follower: input, lstm, blstm, feedforward_*, softmax, or another context layer.
 *
 * Let L, R, D be the three members, B = L + R + 1 and P the preceding layer's size.  The layer's size is B * P,
 * cn_layer_weight_count is 0, and it is neither trainable nor a post output layer.  len_s is the number of rows of slot s in the
 * current fraction whose pattern type is not NONE (a sequence lies in its slot from t = 0 without holes).
 *
 * Forward.  For a real frame (t, s), block b = c / P and unit u = c % P of column c < B * P:
 *      ts           = clamp(t + (b - L) * D, 0, len_s - 1)
 *      out[t][s][c] = x_op[ts][s][u]
 * x_op: what the preceding layer's followers read -- its sum if it is residual, never a dropped or normalised copy.  Units are the
 * reference layout's (blstm: the forward units, then the backward ones): whatever padding the preceding layer's rows have, unit u
 * of block b is column b * P + u of this layer, as cn_layer_read(.., CN_BUF_OUTPUTS, ..) returns it.  The copy is exact in every
 * precision: operand to operand, nothing is rounded (CN_PREC_BF16 behind a feed-forward layer: that layer's bf16 operand copy).
 * Rows that are not real frames (dummy frames, pad slots) are zeros: a feed-forward predecessor's act(bias) on dummy rows never
 * appears.  Edges replicate, as in section Input splicing: a context layer directly behind the input layer produces, bit for bit,
 * what cn_ctx_set_input_splice {L, R, 1} produces for D = 1.
 *
 * Backward.  e is the layer's own outputErrors as its follower wrote them, fp32 in every precision; only real rows are read.  When
 * the preceding layer takes errors -- it is trainable, or a context layer whose own predecessor takes errors -- its outputErrors
 * become, for real frame (ts, s) and unit u,
 *      dx[ts][s][u] = sum over b = 0 .. B-1 (outer, ascending)
 *                     sum over j = 0 .. len_s-1 (inner, ascending) with clamp(j + (b - L) * D, 0, len_s - 1) == ts
 *                         e[j][s][b * P + u]
 * single fp32 additions in exactly that order, starting from +0.0f, without atomics: the result is held to bits and is the same
 * bits from run to run.  Every other row of the preceding layer's outputErrors of the current fraction, and its pad columns, are
 * written as 0.  (For interior ts each b contributes at most one j; only the first and the last frame of a sequence collect runs,
 * of at most max(L, R) * D terms per block.)  Otherwise -- directly behind the input layer, say -- the backward pass does nothing,
 * and the follower's backward pass hands no error back.
 *
 * The follower is any layer that may follow a dense layer: P = B * P of the context layer.  It may drop, normalise, or be residual
 * (when its size is B * P); it reads, normalises or adds the context layer's output like any other predecessor's.  A post output
 * layer directly behind a context layer is refused (it needs a trainable preceding layer).  cn_layer_set_dropout,
 * cn_layer_set_residual, cn_layer_set_layer_norm and the weight entry points refuse a context layer: CN_ERR_BAD_ARG.
 *
 * With no context layer in the net the library launches exactly what it launches without this section and allocates nothing for
 * it. */
/* 0 <= left, right <= 32 and 1 <= dilation <= 16, else CN_ERR_BAD_ARG.  Allocates the layer's outputs and outputErrors, and with the
 * context's first such layer a table of one int per slot.  cn_layer_create(ctx, CN_LAYER_CONTEXT, ...) fails with CN_ERR_BAD_ARG and names this function. */
int  cn_layer_create_context(cn_ctx *ctx, cn_layer *preceding, int left, int right, int dilation, cn_layer **out);
/* The members of a context layer (any pointer may be NULL); a layer of another kind: CN_ERR_BAD_ARG. */
int  cn_layer_context(const cn_layer *layer, int *left, int *right, int *dilation);

/* ---- Strided context layers (Chan et al. 2016, "Listen, Attend and Spell": pyramidal BLSTM; Peddinti et al. 2015: subsampling TDNN;
 * no counterpart in the reference) -------------------------------------------------------------------------------------------------
 * A context layer has a fourth member, the stride S (1 .. 8).  Let L, R, D be its other members, B = L + R + 1, and P the preceding
 * layer's size.  The layer reads its predecessor in the PARENT time axis -- T steps, Tmin, len_s real frames in slot s -- and
 * writes, and every layer behind it runs in, its OWN axis:
 *      n_s = ceil(len_s / S)     T' = ceil(T / S)     Tmin' = ceil(Tmin / S)
 *
 * Forward, for j < n_s, block b = c / P, unit u = c % P:
 *      ts               = clamp(S * j + (b - L) * D, 0, len_s - 1)
 *      out[j][s][b*P+u] = x_op[ts][s][u]
 * Bits are copied, operand to operand, exactly as section Context layers says for S = 1.  Rows j >= n_s below T', pad slots and
 * pad columns are zeros.
 *
 * Pattern types of the new axis, the rule of section Input splicing: FIRST for j = 0, LAST for j = n_s - 1 > 0, NORMAL between,
 * NONE for j >= n_s and for pad slots; the row map is built from them with Tmin' steps of unchecked rows.
 *
 * Targets of the new axis, when the fraction brought any: the target class and target row of frame j are those of parent row
 * S * j, the frame the context is centred on; everything else is -1 / zero rows.  Two strided layers compose:
 * ceil(ceil(len / S1) / S2) = ceil(len / (S1 * S2)), centred on S1 * S2 * j.  A CTC layer reads no per-frame targets; its lengths
 * are n_s, and a sequence with more labels plus adjacent repeats than n_s has no alignment, under the existing rule.
 *
 * Backward.  When the preceding layer takes errors, for every real parent frame (ts, s) and unit u
 *      dx[ts][s][u] = sum over b = 0 .. B-1 (outer, ascending)
 *                     sum over j = 0 .. n_s-1 (inner, ascending) with clamp(S * j + (b - L) * D, 0, len_s - 1) == ts
 *                         e[j][s][b * P + u]
 * single fp32 additions from +0.0f in exactly that order, without atomics: held to bits.  A parent frame that no (b, j) reads gets
 * +0.0 (with L = R = 0 and S = 2: the odd frames).  Every other row of the parent's current fraction, and the pad columns, are
 * written as 0.
 *
 * Everything behind the layer goes by its own axis: T', Tmin' and N' = T' * PSp of every launch, the derived pattern types and row
 * map, the dispatch estimate numSeqs * ((Tmin' + T' + 1) / 2), the LDS sizing of the recurrent kernels, the frame index
 * n = t * PS + ps of the dropout key, the rows of layer norm and residual sums, the slot lengths a later context layer clamps to,
 * the rows of cn_layer_read / cn_layer_write_output_errors (T' * PS rows, as under cn_ctx_set_input_splice), the softmax row
 * statistics, the loss and #correct (summed over the frames the output layer classifies), the CTC sweeps and the default label cap
 * min(max_seq_length of that axis, 512).  Buffers of the followers are sized by ceil(parent max_seq_length / S).  A follower may
 * drop, normalise and be residual exactly as behind a plain context layer; a post output layer directly behind one stays refused.
 *
 * The axis -- slot lengths, pattern types, row map, classes, and the target rows of a post output layer -- is formed once per
 * fraction, on the context's stream, by the strided layer's first forward pass of that fraction; every cn_fraction_load* (a
 * prefetch hit included) makes it stale.  cn_layer_forward, cn_layer_backward, cn_loss_*, cn_layer_read and
 * cn_layer_write_output_errors in an axis that has not been formed for the current fraction fail with CN_ERR_STATE.
 *
 * Stride 1 is the plain context layer: the same launches and the same bits.  With no strided layer in the net the library launches
 * exactly what it launches without this section and allocates nothing for it. */
/* cn_layer_create_context with a stride; 1 <= stride <= 8, else CN_ERR_BAD_ARG.  cn_layer_create_context is the stride-1 call. */
int  cn_layer_create_context_strided(cn_ctx *ctx, cn_layer *preceding, int left, int right, int dilation, int stride, cn_layer **out);
/* 1 for a plain context layer; a layer of another kind: CN_ERR_BAD_ARG. */
int  cn_layer_context_stride(const cn_layer *layer, int *stride);
/* The steps of the current fraction as this layer sees them, and the product of the strides in front of it (any pointer may be
 * NULL); host arithmetic, no synchronisation.  Before a load: CN_ERR_STATE. */
int  cn_layer_time(const cn_layer *layer, int *T, int *Tmin, int *rate);

/* ---- LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning"; no counterpart in the reference) ---------------------
 * A third update family beside the cn_sgd_* and cn_adam_* trios, with the same three entry points and the same protocol: Adam's
 * moments give a direction u per weight, and every LAYER's step is scaled by a trust ratio |w| / |u| of its own, so that the
 * size of a layer's step is about lr times the size of its weights.
 *
 * State.  All state is fp32.  The first moments m live in CN_BUF_WEIGHT_DELTAS and the second moments v in
 * CN_BUF_ADAM_SECOND_MOMENTS, as under Adam (zero at the first call unless uploaded); cn_buffer does not change.  The direction u
 * is one scratch vector of the arena's length, an allocation of its own made by the first LAMB call together with one small
 * record per trainable layer.  A context belongs to the family of its first update or arm call: LAMB after Adam or steepest
 * descent, or the reverse, fails with CN_ERR_STATE.  The library keeps no clock: `step` (>= 1) is the caller's count of updates.
 *
 * Host scalars.  From the float arguments the host forms, in double, rounded once to float,
 *      omb1 = 1 - beta1      omb2 = 1 - beta2
 *      c_t   = sqrt(1 - beta2^step) / (1 - beta1^step)
 *      eps_t = eps * sqrt(1 - beta2^step)
 * (Adam's alpha_t is lr * c_t; here lr stays outside the quotient, because the trust ratio multiplies it.)
 *
 * Pass 1, per arena entry i of a layer (i counted from the layer's first entry; n, the layer's padded count, is its weight count
 * rounded up to a multiple of four by pad entries that are zero).  Every operation is a single fp32 operation rounded to nearest:
 * no contraction, correctly rounded sqrt and division, denormals kept.  g is the layer's weightUpdates entry as the clipping
 * record hands it over (g' = mul_rn(scale, g) on a clipped step, see Gradient clipping).
 *      m = beta1*m + omb1*g          v = beta2*v + omb2*(g*g)            (the operations of Adam, in the same order)
 *      r = div_rn(mul_rn(c_t, m), add_rn(sqrt_rn(v), eps_t))
 *      u = decays(i) ? add_rn(r, mul_rn(decay, w)) : r
 * decays(i) is the set the Weight decay section names (input and recurrent weights; never bias, peephole or pad entries), and
 * `decay` is the context's cn_ctx_set_weight_decay coefficient itself, not ld.  Under LAMB the decay term enters the direction,
 * as in the paper: the w0 = w - ld*w rule of the Weight decay section is NOT applied.  With decay 0 no operation is performed
 * for it.
 *
 * The two sums, per layer.  Sw = sum of w[i]^2 over the weights as they stood before the step, Su = sum of u[i]^2, i = 0 .. n-1.
 * Both are formed in DOUBLE (each square formed in double from the float, so exact), in exactly the order the Gradient clipping
 * section states for S, applied to the layer's n entries: L = 16384 lanes, ascending within a lane, then fourteen pairwise levels
 * over neighbouring lanes.  The order depends on i and n alone -- not on the grid, the CU count, the precision mode or the
 * "deterministic" option.
 *
 * Ratio and step.
 *      nw = (float) sqrt(Sw)       nu = (float) sqrt(Su)                 (correctly rounded double sqrt, rounded once to float)
 *      ratio = 1                                   if nw == 0, nu == 0, or Sw or Su is not finite
 *      ratio = div_rn(nw, nu), then raised to min_ratio if below it
 *                              and lowered to max_ratio if above it (max_ratio != 0)      otherwise
 *      step  = mul_rn(lr_layer, ratio)
 *      w     = sub_rn(w, mul_rn(step, u))          for every entry of the layer
 * lr_layer is the call's rate or the layer's own (cn_layer_set_learning_rate).  {ratio, nw, nu} is the layer's record
 * (cn_layer_trust_ratio).  A non-finite gradient without clipping poisons m as under Adam; set a clipping bound
 * (cn_ctx_set_grad_clip, the driver's --max_grad_norm) to have such a step skipped.  A step the clipping record skips leaves
 * w, m, v, the layer's record and the operand copies bit for bit as they were.
 *
 * Interactions.  Batch learning updates once per epoch sum (cn_ctx_take_accumulated, then the update).  Weight noise and weight
 * averaging see the updated weights as the weights.  Data-parallel: every rank forms the same sums of the same reduced gradient in
 * the same order, so the replicas stay bit-identical without an exchange.  Armed updates: the direction pass writes a layer's m
 * and v before the layer's ratio is known, so an armed LAMB step is accepted and checked and then applied by the completing
 * cn_lamb_update_all or per-layer cn_lamb_update call (which must name the armed values, else CN_ERR_STATE) -- the deferral
 * clipping uses; the overlap of the update with the backward pass is lost.  While the weights are swapped with their average the
 * calls fail with CN_ERR_STATE like the other update calls.  Argument errors as for Adam.
 *
 * Without any LAMB call the library launches exactly what it launches today and allocates nothing for this section. */
/* beside cn_adam_update: the LAMB step of one layer (its own sums, its own ratio) at `learning_rate` as given */
int  cn_lamb_update(cn_layer *layer, float learning_rate, float beta1, float beta2, float eps, int64_t step);
/* beside cn_adam_update_all: every trainable layer -- one direction launch and one apply launch for all of them, then the operand
 * copies; a layer with a learning rate of its own takes it as its lr_layer.  Orders itself behind cn_allreduce_grads. */
int  cn_lamb_update_all(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step);
/* beside cn_ctx_arm_adam: accepted and checked; the step is applied by the completing call (see Armed updates above) */
int  cn_ctx_arm_lamb(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step);
/* The bounds of every layer's ratio; a fresh context has 0 and 0, and max_ratio = 0 means no upper bound.  Negative, NaN, infinite,
 * or min_ratio > max_ratio with max_ratio != 0: CN_ERR_BAD_ARG.  While an armed update is pending: CN_ERR_STATE. */
int  cn_ctx_set_trust_bounds(cn_ctx *ctx, float min_ratio, float max_ratio);
int  cn_ctx_get_trust_bounds(const cn_ctx *ctx, float *min_ratio, float *max_ratio);
/* The record of the layer's last LAMB step that was not skipped: *ratio (bounds applied), *weight_norm = nw, *update_norm = nu; 1, 0, 0
 * before the first.  Any pointer may be NULL.  A layer without weights: CN_ERR_BAD_ARG.                              [sync] */
int  cn_layer_trust_ratio(cn_layer *layer, float *ratio, float *weight_norm, float *update_norm);

/* ---- CTC decoding (no counterpart in the reference; Graves et al. 2006, section 3.2: best path decoding) -------------------------
 * What a CN_LAYER_CTC layer recognises in the posteriors of the softmax layer in front of it, and how far that is from the
 * label sequences cn_layer_set_label_sequences brought: integer work on the fp32 posteriors where they lie, nothing is copied to
 * the host but the results.  Prefix search and language models are not part of it.
 *
 * The rule, for slot s of the loaded fraction, len_s its length in the ctc layer's own time axis (cn_layer_time; behind strided
 * context layers the reduced length), C the layer's size, blank = C - 1:
 *      k_t     = the index of the largest of the C posteriors of frame t; of equal values the LOWEST index wins (the scan
 *                `best = 0; for k = 1 .. C-1: if (y[k] > y[best]) best = k`, which is numpy.argmax).  Pad columns, pad slots and
 *                frames t >= len_s take no part.
 *      decoded = k_t for t = 0 .. len_s - 1, kept when k_t != blank and (t == 0 or k_t != k_{t-1}), in order: D_s labels.
 *                `x _ x` keeps both x; a run of x is one x however long.
 *      dist_s  = the Levenshtein distance of decoded to the slot's U_s labels with unit costs for an insertion, a deletion and a
 *                substitution; D_s for U_s = 0 and U_s for D_s = 0.
 * All three are integers: two runs, and any order of summation, give the same numbers.
 *
 * Bounds.  No bound on the steps T.  The distance keeps three anti-diagonals of min(D_s, U_s) + 1 ints in LDS, at most 60 KB:
 * min(T, longest label sequence of the fraction) <= 5119, else CN_ERR_SHAPE; nothing is ever truncated.  A ctc layer's label cap
 * cannot exceed 2047 (cn_layer_set_label_sequences), so no fraction a layer accepts comes near the bound.
 *
 * Errors of all three calls: a layer that is not ctc: CN_ERR_BAD_ARG; before a fraction is loaded, and before the softmax layer in
 * front has run its forward pass of the loaded fraction: CN_ERR_STATE.  The first decoding call of a layer allocates its buffers
 * (2 * max_seq_length * padded parallel sequences ints); without one the library launches what it launches without this section. */
/* decoded [num_sequences][T] with T the layer's own steps (cn_layer_time) -- only the first decoded_lengths[s] entries of row s are
 * defined --, decoded_lengths [num_sequences], distances [num_sequences]; any of the three may be NULL.  distances[s] is -1 for
 * every s when the loaded fraction has no valid label sequences (a forward pass over unlabelled data); decoding works all the
 * same.                                                                                                              [sync] */
int  cn_ctc_decode(cn_layer *ctc, int *decoded, int *decoded_lengths, int *distances);
/* Beside cn_loss_accumulate: adds the sum of dist_s and the sum of U_s over the fraction's slots to two 64-bit integer sums on the
 * device that the context keeps.  Without valid label sequences: CN_ERR_STATE.                                      [async] */
int  cn_ctc_decode_accumulate(cn_layer *ctc);
/* Beside cn_loss_read: the two sums (either pointer may be NULL; both 0 before the first accumulation); `reset` != 0 clears them
 * behind the read.  Data-parallel: the sums of this rank's sequences.                                                [sync] */
int  cn_ctc_decode_read(cn_ctx *ctx, int64_t *label_errors, int64_t *labels, int reset);

#ifdef __cplusplus
}
#endif
#endif /* CURRENNT_HIP_H */
