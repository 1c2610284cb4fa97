// C ABI of libcurrennt_hip.so (include/currennt_hip.h): contexts, layer objects, buffer ownership
// and the per-layer kernel sequences.  Host-only code; all device work is in the .hip files.
//
// Layer call sequences follow the reference methods they replace:
//   LSTM   forward  LstmLayer.cu:763-886    backward LstmLayer.cu:888-1051
//   FF     forward  FeedForwardLayer.cu:143-170   backward :172-224
//   softmax forward SoftmaxLayer.cu:250-315 backward :317-353
//   post output     MulticlassClassificationLayer.cu:159-240, SsePostOutputLayer.cu:114-155
#include "cn_internal.h"
#include "cn_noise_unpack.h"
#include "../../include/currennt_hip_debug.h"

#include <dlfcn.h>
#include <rccl/rccl.h>       // types and prototypes only: librccl is opened with dlopen (struct Rccl below), never linked

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

using namespace cn;

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
namespace {

thread_local std::string g_last_error;

struct cn_error : std::runtime_error {
    int code;
    cn_error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

void hip_check(hipError_t e, const char *what)
{
    if (e != hipSuccess)
        throw cn_error(CN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_CHECK(x) hip_check((x), #x)

template <typename F> int guarded(F &&f)
{
    try { f(); return CN_OK; }
    catch (const cn_error &e) { g_last_error = e.what(); return e.code; }
    catch (const std::exception &e) { g_last_error = e.what(); return CN_ERR_HIP; }
}

// a device temporary of one call: freed on every way out of it, a throw included
struct Scratch {
    void *p = nullptr;
    Scratch() = default;
    explicit Scratch(size_t bytes) { alloc(bytes); }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (p) (void)hipFree(p); }
    void alloc(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes)); }
    template <typename T = float> T *get() const { return (T *)p; }
};

// The optimizer's rule of an update: momentum SGD (lr, mom) or Adam (lr, b1, b2, eps, step); lr is the caller's learning rate,
// a layer with a rate of its own replaces it (layer_lr).  decay: the context's weight decay in force when the call came in, or, of
// an armed rule, when it was armed (cn_ctx_set_weight_decay; 0: off) -- the caller's arguments do not name it, so same_rule
// does not compare it.  lamb (include/currennt_hip.h, section LAMB): Adam's arguments and moments (adam is set too), the layer-wise
// trust ratio on top
struct UpdateRule { bool adam = false, lamb = false; float lr = 0.f, mom = 0.f, b1 = 0.f, b2 = 0.f, eps = 0.f; int64_t step = 0; float decay = 0.f; };
bool same_rule(const UpdateRule &a, const UpdateRule &b)
{
    if (a.adam != b.adam || a.lamb != b.lamb) return false;
    return a.adam ? a.lr == b.lr && a.b1 == b.b1 && a.b2 == b.b2 && a.eps == b.eps && a.step == b.step
                  : a.lr == b.lr && a.mom == b.mom;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// objects
// ---------------------------------------------------------------------------------------------
// The time axis a layer runs on (include/currennt_hip.h, section Strided context layers): the steps of the current fraction, the
// pattern types inside an allocation with guard steps and the row map behind them (cn_ctx::pat_bytes), the estimate of the real
// frames, the classes, and the slot lengths.  The context owns the base axis, a mirror of its own members (sync_base); every
// strided context layer owns one more, formed on the context's stream by its first forward pass of a fraction (serial: of load
// number cn_ctx::frac_serial).  Every layer reaches its axis through cn_layer::ax.
struct TimeAxis {
    int T = 0, Tmin = 0, N = 0, Next = 0, maxT = 0;
    int rate = 1;                                     // product of the strides in front of the axis
    char *pat = nullptr, *pat_raw = nullptr;
    size_t pat_maxN = 0, pat_guard = 0;
    int est_real = 0;
    int *tcls = nullptr;
    int *len = nullptr;                               // [PSp] real frames per slot (the base axis: cn_ctx::cx_len, formed on demand)
    uint64_t serial = 0;
    cn_layer *owner = nullptr;                        // the strided layer that forms the axis (nullptr: the base axis)
    int *rowmap() const { return pat_raw ? (int *)(pat_raw + ((pat_maxN + 2 * pat_guard + 15) & ~(size_t)15)) : nullptr; }
};

struct cn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // side stream: weight-gradient GEMMs run beside the next layer's (latency-bound, 26-CU) recurrent kernel
    hipStream_t side = nullptr;
    // CU-masked twin of the side stream: gradient GEMMs that run beside a recurrent kernel have its whole duration
    // to finish, and at full speed their memory traffic stalls the latency-bound recurrent kernel (291 vs 229 us
    // per backward launch); on a subset of the CUs they run longer but draw less bandwidth
    hipStream_t side_slow = nullptr; int side_cus = 0;    // CU-masked side stream and its CU count
    int tn_cus = 0;                       // CUs the gradient products of the current on_side() call may fill (0 = the chip)
    hipEvent_t ev_sgd = nullptr, ev_ext = nullptr;
    hipEvent_t ev_pack_last = nullptr;         // = ev_pack of the last layer whose operand copies cn_sgd_update_all rebuilt (not owned)
    std::vector<hipEvent_t> pending_joins;     // side-stream work the main stream has not waited for yet ...
    std::vector<hipStream_t> pending_join_streams;   // ... and the stream each event was recorded on (same index)
    bool overlap = true;
    bool attach_forks = true;                  // CN_NO_ATTACHED_FORKS=1: fork / join / update events recorded with hipEventRecord
    bool f32 = true;                           // operands are fp32 in memory (CN_PREC_F32 and CN_PREC_BF16X3)
    // option "deterministic": every sum over the patterns of a fraction (weight gradients, bias / peephole / column sums, the
    // error) is formed in a fixed order -- partials stored by their producers, added by one thread per output -- instead of
    // with fp32 atomics in arrival order: two runs give bit-identical weights, as the reference's Cpu path does (one logical
    // thread per weight, serial sum: LstmLayer.cu:289-512, FeedForwardLayer.cu:82-102).  On by default in the parity modes
    // (CN_PREC_F32, CN_PREC_BF16X3), opt-in for CN_PREC_BF16; CN_DETERMINISTIC=0/1 sets the default of new contexts.
    bool det = false;
    Options opt;                               // A/B and test switches (cn_internal.h): the environment's at creation, cn_ctx_set_option afterwards
    int prec = P_F32;                          // arithmetic of the MFMA products: P_F32 / P_BF16 / P_X3 (cn_internal.h)
    int num_cus = 256;                         // hipDeviceProp_t::multiProcessorCount of the bound device
    std::string arch;
    std::vector<cn_layer *> layers;

    // current fraction (Layer::loadSequences, Layer.cpp:134-141)
    // PS: parallel sequences as the caller sees them; PSp >= PS: sequence slots per time step on the
    // device (padded to the recurrent kernels' sequence-group size; pad slots are permanent dummies).
    // N = T*PSp frames on the device, Next = T*PS frames in host layouts.
    int PS = 0, PSp = 0, rpl = 1, maxT = 0, T = 0, Tmin = 0, N = 0, Next = 0, numSeqs = 0;
    bool loaded = false;
    char *d_pat = nullptr, *d_pat_raw = nullptr;      // [maxN] pattern types inside an allocation with guard steps
    // ... and behind them the fraction's row map (GemmNT::rowmap; launch_rowmap): one allocation, so that the map travels with the
    // pattern types when a prefetched fraction's buffers are swapped in
    size_t pat_maxN = 0, pat_guard = 0;
    static size_t pat_bytes(size_t maxN, size_t guard) { return ((maxN + 2 * guard + 15) & ~(size_t)15) + (4 + 2 * maxN) * sizeof(int); }
    int *rowmap_of(char *pat_raw) const { return pat_raw ? (int *)(pat_raw + ((pat_maxN + 2 * pat_guard + 15) & ~(size_t)15)) : nullptr; }
    int est_real = 0;                                 // estimate of the current fraction's real frames (dispatch only)
    // context layers (include/currennt_hip.h, section Context layers): len_s of every slot [PSp], allocated with the first such
    // layer and formed on the device by the first context layer's pass over a fraction (cx_serial: of load number frac_serial)
    uint64_t frac_serial = 0, cx_serial = 0;
    int *cx_len = nullptr;
    int *d_tcls = nullptr;
    float *d_loss = nullptr;      // [2] per-call (error, #correct as int bits)
    float *d_loss_acc = nullptr;  // [2] running sums for cn_loss_accumulate
    unsigned long long *d_ctc_sums = nullptr;   // {label errors, labels} of cn_ctc_decode_accumulate, allocated by the first decoding call
    unsigned long long *d_xch = nullptr; size_t xch_bytes = 0;   // cluster kernels' exchange granules
    unsigned xch_epoch = 0;       // granule tags handed out so far (LstmRec::xch_epoch)
    int *d_fault = nullptr;       // device fault word (bounded spins)
    float *d_colpart = nullptr;   // softmax_mcc_bwd_colpart_floats(): replicas of the output layer's column sums (zero between launches)
    float *d_rowstat = nullptr;   // [maxN][2] per-pattern {log p_target, correct} of the last softmax forward pass
    cn_layer *rowstat_of = nullptr;
    bool loss_deferred = false;   // cn_loss_accumulate of the current fraction has not been enqueued yet: it rides on the output
                                  // layer's backward launch (softmax_mcc_bwd_kernel) or is flushed by whoever needs the sums / the rows

    // host fractions (cn_fraction_load): packed into pinned memory, uploaded on a copy stream into one of two
    // device staging areas while the previous fraction still computes, re-laid out by fraction_load_kernel
    hipStream_t copy = nullptr;
    char *h_stage[2] = {nullptr, nullptr}, *d_stage[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    unsigned upload_idx = 0;

    // cn_fraction_prefetch_resident: the announced fraction is re-laid out into the alternate buffers on the side stream of
    // the next gradient work (beside the backward pass); the load that follows swaps the buffers instead of running the kernel
    struct Prefetch {
        bool valid = false, launched = false;
        cn_fraction f{}; cn_layer *input = nullptr, *post = nullptr;
        int hits = 0;                                            // loads that found their fraction re-laid out (cn_dbg_prefetch_hits)
        bool host = false; cn_fraction f_host{}; int slot = 0;     // cn_fraction_prefetch: f points into staging area `slot`, f_host is what the caller announced
        char *pat = nullptr, *pat_raw = nullptr; int *tcls = nullptr; void *in_op = nullptr; float *targets = nullptr;   // alternates
        bool allocated = false;
        cn_input_augment aug{};                                  // the augmentation in force at the prefetch (all zero: off)
        cn_input_splice splice{};                                // ... and the splice settings (all zero: off)
        int *aug_tab = nullptr;                                  // its slot table: this re-layout runs on the side stream
    } pf;

    // cn_ctx_set_input_augment (include/currennt_hip.h, section Input augmentation): the settings the loads that follow go by --
    // all zero when off, so that two settings compare member by member -- and the slot table of the loads on this stream
    // ([PS][AUG_TAB_STRIDE] ints, allocated by the first enabling call that knows PS)
    cn_input_augment aug{};
    int *aug_tab = nullptr;
    // cn_ctx_set_input_splice (section Input splicing and frame skipping): all zero when off (frame_skip >= 1: on), so that two
    // settings compare member by member.  A spliced load forms its slot lengths in the same table (aug_tab).
    cn_input_splice splice{};

    // data-parallel training: RCCL communicator of this rank, its stream and the newest reduction's event
    ncclComm_t comm = nullptr;
    IpcComm *ipc = nullptr;                    // CN_COMM_BACKEND=ipc: the test backend (cn_comm_ipc.cpp) in place of RCCL
    int comm_rank = 0, comm_world = 0;
    bool has_comm() const { return comm != nullptr || ipc != nullptr; }
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_comm = nullptr, ev_comm_fork = nullptr;
    bool comm_pending = false;
    int64_t comm_exchanges = 0;                // all-reduces enqueued by cn_allreduce_grads (cn_comm_backend)

    // cn_ctx_arm_update / cn_ctx_arm_adam: the step of the coming backward pass (rule `arm`) is applied layer by layer, as soon as
    // a layer's own gradient is complete (on the stream that computed it), instead of for all layers behind the last backward kernel
    bool armed = false;
    UpdateRule arm;
    // Optimizer family of the context's first update / arm call (0: none yet).  weightDeltas is the momentum term under one and the
    // first moment under the other, so a context stays with its family.
    enum { FAMILY_NONE = 0, FAMILY_SGD, FAMILY_ADAM, FAMILY_LAMB };
    int family = FAMILY_NONE;
    float *adam_v = nullptr;              // Adam's second moments, [total] like a part of the arena, zeroed; allocated at the first Adam call
    // LAMB (include/currennt_hip.h, section LAMB): the direction u, [total] like a part of the arena, and one record per trainable
    // layer (cn_layer::lamb_rec), both allocated at the first LAMB call; the trust bounds (cn_ctx_set_trust_bounds; 0 / 0: none)
    float *lamb_u = nullptr;
    LambRecord *lamb_recs = nullptr;
    float trust_min = 0.f, trust_max = 0.f;

    // Weight averaging (include/currennt_hip.h, section Weight averaging): the average, [total] like a part of the arena, allocated
    // by the first averaging step (which copies the weights) or the first upload (a copy of the weights, then the layer's part);
    // avg_swapped: the weights part of the arena holds the average and `avg` the raw weights right now
    float *avg = nullptr;
    bool avg_swapped = false;

    // cn_ctx_set_grad_clip (include/currennt_hip.h, section Gradient clipping): the bound (0: off), the device record -- allocated
    // by the first non-zero bound -- and whether the record still holds the norm of what weightUpdates holds now (cleared by
    // everything that changes the gradient; the first update call behind that forms the norm again)
    float clip_max = 0.f;
    // cn_ctx_set_weight_decay (section Weight decay): the coefficient of the update calls that follow (0: off).  Only a number: an
    // update call copies it into its rule (UpdateRule::decay), an arming call into `arm`.
    float decay = 0.f;
    ClipRecord *clip_rec = nullptr;
    bool clip_valid = false;
    // ... an armed step cannot run layer by layer behind a GLOBAL norm: with clipping on, arming only records the rule (`arm`) and
    // the completing *_update* call applies the step.  Layers whose completing per-layer call is still to come: cn_layer::deferred.
    bool arm_deferred = false;

    // cn_ctx_set_dropout_pass: whether the forward passes that follow drop, and the caller's (seed, pass) of their masks
    bool drop_enable = false;
    uint64_t drop_seed = 0, drop_pass = 0;
    int next_ordinal = 0;                 // layers created so far (cn_layer::ordinal)

    // cn_ctx_set_weight_noise (include/currennt_hip.h, section Weight noise): the triple the backward passes that follow go by
    float noise_sigma = 0.f;              // 0: off
    uint64_t noise_seed = 0, noise_pass = 0;
    // option noise_ahead: the sets were generated on the side stream beside the forward pass; ev_noise completes with them and
    // the first backward pass that reads a set makes the main stream wait for it (noise_wait)
    hipEvent_t ev_noise_fork = nullptr, ev_noise = nullptr;
    bool noise_wait = false;

    // parameter arena [weights | weightUpdates | weightDeltas]
    bool finalized = false;
    float *arena = nullptr;
    float *acc = nullptr;                 // epoch sum of weightUpdates (batch learning, cn_ctx_accumulate_updates); [total]
    bool acc_valid = false;
    size_t total = 0;

    // timing
    bool timing = false;
    int rpl_override = 0;
    struct Span { hipEvent_t a, b; };
    std::vector<Span> spans[KC_COUNT];
    std::vector<hipEvent_t> free_events;
    double acc_ms[KC_COUNT] = {};
    long acc_n[KC_COUNT] = {};

    size_t esz() const { return f32 ? 4 : 2; }

    TimeAxis base;                        // the axis of the input layer and of everything in front of the first strided layer
};

struct cn_layer {
    cn_ctx *ctx = nullptr;
    cn_layer_kind kind = CN_LAYER_INPUT;
    cn_layer *prev = nullptr;
    int size = 0;
    float bias = 0.f;
    int PS = 0, PSp = 0, maxT = 0;
    bool trainable = false, post = false, lstm = false, has_follower = false;
    bool mcc_pending = false;             // softmax layer: multiclass error injection deferred into the fused backward kernel
    // wide softmax layer (softmax_fwd_can_be_lazy): the forward pass may leave the LOGITS in out_f32 and {offset, sum} per row in
    // sm_stat; the fused backward kernel recomputes the posteriors from them, anybody else gets them through posteriors()
    float *sm_stat = nullptr;
    bool sm_lazy = false;                 // out_f32 holds logits right now
    bool sm_lazy_next = true;             // the last forward pass's posteriors were only consumed by the fused backward kernel
    bool sm_read = false;                 // somebody else looked at them since the forward pass

    int dirs = 1, H = 0, Hp = 0;          // lstm geometry
    int Lp = 0;                           // padded output width (row stride of out/err)
    int P = 0, Pp = 0;                    // preceding layer size / padded width

    // activations
    void *out_op = nullptr;               // [maxN][Lp] operand copy of the outputs
    float *out_f32 = nullptr;             // [maxN][Lp] fp32 outputs (ff/softmax; aliases out_op in f32 mode)
    float *err = nullptr;                 // [maxN][Lp] outputErrors
    float *stage_in = nullptr;            // input layer: [maxN][size] fp32 as loaded
    float *targets = nullptr;             // sse: [maxN][size]

    // dropout on this layer's input (include/currennt_hip.h, section Dropout)
    int ordinal = 0;                      // index in the context's creation order: part of the mask's key
    float drop_rate = 0.f;                // cn_layer_set_dropout
    void *in_drop = nullptr;              // [maxN][Pp] masked operand copy of prev->out_op, allocated at the first non-zero rate
    bool dropped = false;                 // the last forward pass dropped ...
    DropArgs drop{};                      // ... with this key: what its backward pass masks the handed-back error with

    // layer normalization of this layer's input (include/currennt_hip.h, section Layer normalization)
    bool layer_norm = false;              // cn_layer_set_layer_norm
    float ln_eps = 1e-5f;
    void *in_norm = nullptr;              // [maxN][Pp] (op) normalised copy of what the preceding layer's followers read; allocated when first enabled
    float *ln_rstd = nullptr;             // [maxN] 1 / sqrt(var + eps) of every row of the last forward pass
    bool normed = false;                  // the last forward pass normalised ...
    LnArgs ln{};                          // ... with this eps and geometry: what its backward pass goes by

    // residual connection around this layer (include/currennt_hip.h, section Residual connections)
    bool residual = false;                // cn_layer_set_residual
    void *res_sum = nullptr;              // [maxN][Lp] (op) out_op + what the preceding layer's followers read; allocated when first enabled
    float *res_e = nullptr;               // dense layers: [maxN][Lp] the outputErrors as handed in (launch_ff_delta overwrites err in place)
    bool summed = false;                  // the last forward pass summed ...
    ResArgs res{};                        // ... with this geometry: what its followers read and what its backward pass adds go by the record

    // context layer (include/currennt_hip.h, section Context layers): its members, and the geometry of its last forward pass,
    // which its backward pass goes by
    bool context = false;
    int cx_left = 0, cx_right = 0, cx_dil = 1;
    ContextArgs cx{};
    // ... with a stride above 1 (section Strided context layers): the layer reads its predecessor in that layer's axis and owns
    // the axis it writes in and its followers run in
    int cx_stride = 1;
    TimeAxis own_axis;
    // the time axis this layer's rows lie in: the context's base axis, or that of the nearest strided layer in front (or this one)
    TimeAxis *ax = nullptr;
    // post output layer behind a strided layer: the target rows of its axis, gathered from `targets` (which the loads fill at the
    // base rate) by the first use in a fraction
    float *ax_targets = nullptr;
    uint64_t ax_targets_serial = 0;

    // lstm internals
    float *acts = nullptr, *cell = nullptr, *th = nullptr;
    void *pre16 = nullptr;                // bf16 mode: the input projection's pre-activations as bf16 (LstmRec::pre16), where the forward kernel takes them
    bool err_in_delta = false;            // ff/softmax, bf16 mode: outputErrors of the last backward pass exist only as the bf16 operand copy
    void *delta_op = nullptr;

    // parameters (flat reference layout, inside the ctx arena)
    size_t woff = 0;
    int nw = 0;
    int lamb_rec = -1;                    // index of the layer's LambRecord (ensure_lamb)
    float *w = nullptr, *wu = nullptr, *wd = nullptr;
    float own_lr = -1.f;                  // JSON "learningRate" (TrainableLayer.cu:58); negative: the optimizer's
    std::vector<float> pending_w;         // set_weights before the arena exists
    bool dirty = true;                    // packed copies out of date
    bool updated = false;                 // armed update: this layer's step has been enqueued behind its gradient already
    bool deferred = false;                // armed with clipping on (cn_ctx::arm_deferred): the completing call has not come yet

    // packed copies
    void *Win = nullptr, *WinT = nullptr, *Wrec = nullptr, *WrecT = nullptr;
    float *bias_p = nullptr, *peep_p = nullptr;
    // weight noise: the noisy set of the copies a backward pass reads (WinT, and WrecT / peep_p of an LSTM layer), allocated by the
    // first backward pass with a non-zero sigma.  noisy_ready: the set holds the noise of the triple in force and of the weights as
    // they are, and this layer's backward pass has not consumed it yet; noise_used: the last backward pass read the set.
    void *nWinT = nullptr, *nWrecT = nullptr;
    float *npeep = nullptr;
    bool noisy_ready = false, noise_used = false;
    float *grad_block = nullptr;         // dWin | dWrec | dbias | dpeep  (or dW | colsum), zeroed per backward
    size_t grad_block_floats = 0;
    float *dWin = nullptr, *dWrec = nullptr, *dbias = nullptr, *dpeep = nullptr;

    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_pack = nullptr;         // operand copies rebuilt on the side stream after cn_sgd_update_all
    bool pack_pending = false;

    char kname[2][CN_KNAME_LEN] = {{0}, {0}};   // recurrent kernels the last forward / backward pass launched (written by the launchers)

    // deterministic mode (allocated at the first backward pass that needs them)
    float *det_ws = nullptr;              // split-K partial products: DET_MAX_SPLITS copies of [dWin | dWrec]
    float *gpart = nullptr; int gpart_slots = 0;   // LSTM: per-workgroup bias / peephole sums (LstmRec::gpart)
    float *det_colpart = nullptr;         // dense layers: per-workgroup column sums (det_colsum_part_floats)

    // CTC post output layer (cn_ctc.hip): label sequences of the fraction loaded last, the sweeps' workspace
    int ctc_cap = 0;                      // labels per sequence the buffers were sized for (option ctc_max_labels at creation)
    int *ctc_labels = nullptr;            // [labels | next | first], ctc_stride ints each (the fraction's label total), then laboff [PSp + 1]
    size_t ctc_stride = 1;
    bool ctc_labels_valid = false;        // set by cn_layer_set_label_sequences, cleared by every cn_fraction_load*
    bool ctc_swept = false;               // the sweeps of the current forward pass have been enqueued (error and output errors share them)
    int ctc_maxS = 1;                     // 2 * (longest label sequence of the fraction) + 1
    int2 *ctc_alpha = nullptr, *ctc_beta = nullptr; int ctc_Sp = 0;
    int *ctc_info = nullptr;
    float *ctc_rowstat = nullptr;         // [PSp][2]: {-log p, 1} or {0, 0} per slot
    // two pinned images of ctc_labels, used in turn (the host packs fraction k + 1 while the upload of fraction k may still be
    // queued); an image's last upload has read it when its event completes
    int *ctc_hbuf[2] = {nullptr, nullptr}; hipEvent_t ctc_ev[2] = {nullptr, nullptr}; unsigned ctc_uploads = 0;
    // CTC decoding (cn_ctc_decode.hip), allocated by the layer's first decoding call: [maxN] argmax per row, then [PSp][maxT]
    // decoded, [PSp] lengths, [PSp] distances
    int *ctc_dec = nullptr;
    uint64_t fwd_serial = 0;              // softmax layer: the load number (cn_ctx::frac_serial) of its last forward pass

    std::vector<void *> owned;            // device allocations to free

    size_t maxN() const { return (size_t)PSp * maxT; }
};

// ---- options (cn_internal.h) -------------------------------------------------------------------
namespace cn {
static const Options &default_options() { static const Options o = options_from_env(); return o; }
static thread_local const Options *t_opt = nullptr;
const Options &opt() { return t_opt ? *t_opt : default_options(); }
Options options_from_env()
{
    Options o;
    auto env_name = [](const char *name) { std::string e = "CN_"; for (const char *p = name; *p; ++p) e += (char)toupper((unsigned char)*p); return e; };
#define CN_OPT_FLAG(name) o.name = getenv(env_name(#name).c_str()) != nullptr;
#define CN_OPT_NUM(name, dflt) if (const char *v = getenv(env_name(#name).c_str())) o.name = atol(v);
    CN_OPTION_LIST(CN_OPT_FLAG, CN_OPT_NUM)
#undef CN_OPT_FLAG
#undef CN_OPT_NUM
    return o;
}
bool option_set(Options &o, const char *name, long value)
{
#define CN_OPT_FLAG(n) if (!strcmp(name, #n)) { o.n = value != 0; return true; }
#define CN_OPT_NUM(n, dflt) if (!strcmp(name, #n)) { o.n = value; return true; }
    CN_OPTION_LIST(CN_OPT_FLAG, CN_OPT_NUM)
#undef CN_OPT_FLAG
#undef CN_OPT_NUM
    return false;
}
bool option_get(const Options &o, const char *name, long *value)
{
#define CN_OPT_FLAG(n) if (!strcmp(name, #n)) { *value = o.n; return true; }
#define CN_OPT_NUM(n, dflt) if (!strcmp(name, #n)) { *value = o.n; return true; }
    CN_OPTION_LIST(CN_OPT_FLAG, CN_OPT_NUM)
#undef CN_OPT_FLAG
#undef CN_OPT_NUM
    return false;
}
}  // namespace cn

namespace {

// the base axis mirrors the context's own members: behind everything that sets or swaps them
void sync_base(cn_ctx *c)
{
    TimeAxis &b = c->base;
    b.T = c->T; b.Tmin = c->Tmin; b.N = c->N; b.Next = c->Next; b.maxT = c->maxT; b.rate = 1;
    b.pat = c->d_pat; b.pat_raw = c->d_pat_raw; b.pat_maxN = c->pat_maxN; b.pat_guard = c->pat_guard;
    b.est_real = c->est_real; b.tcls = c->d_tcls; b.len = c->cx_len; b.serial = c->frac_serial; b.owner = nullptr;
}

// every entry point that touches the device: bind it and make the context's options the ones the launch paths see
void enter(cn_ctx *c)
{
    HIP_CHECK(hipSetDevice(c->device));
    cn::t_opt = &c->opt;
    // the mirror is hand-kept: whoever assigns or swaps one of the mirrored members and forgets sync_base is told at the next call
    const TimeAxis &b = c->base;
    if (b.T != c->T || b.Tmin != c->Tmin || b.N != c->N || b.Next != c->Next || b.maxT != c->maxT || b.pat != c->d_pat ||
        b.pat_raw != c->d_pat_raw || b.pat_maxN != c->pat_maxN || b.pat_guard != c->pat_guard || b.est_real != c->est_real ||
        b.tcls != c->d_tcls || b.len != c->cx_len || b.serial != c->frac_serial)
        throw cn_error(CN_ERR_STATE, "internal: the base time axis is out of date (a member of the context changed without sync_base)");
}

void *dalloc(cn_layer *l, size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0) bytes = 16;
    HIP_CHECK(hipMalloc(&p, bytes));
    HIP_CHECK(hipMemsetAsync(p, 0, bytes, l->ctx->stream));
    l->owned.push_back(p);
    return p;
}

// A per-frame buffer of an LSTM layer with CN_GUARD_STEPS time steps of zeros in front of frame 0 and behind frame maxN: the
// hand-written recurrent loops (cn_lstm_s2.hip) prefetch several steps ahead in EVERY step, also in the last ones, where the
// target lies outside [0, T) -- those loads must hit mapped memory, their values are never used.  (Nobody writes the guards:
// every kernel addresses frames 0 .. N-1 from the returned pointer.)
void *dalloc_guarded(cn_layer *l, size_t bytes, size_t bytes_per_step)
{
    const size_t guard = (size_t)CN_GUARD_STEPS * bytes_per_step;
    return (char *)dalloc(l, bytes + 2 * guard) + guard;
}

// ---- CU-masked stream ------------------------------------------------------------------------
// One CU-masked stream per (device, CU count) for the life of the process, shared by every context on that device.
// hipStreamDestroy of such a stream is not reliable on ROCm 7.2: depending on the network (seen with 2, 4, 5 and 6
// layers of blstm1024, not with the headline topology) it never returned although hipStreamSynchronize and
// hipStreamQuery reported the stream idle, with or without a hipDeviceSynchronize in front.  Contexts order their own
// work on it with events, so sharing it costs at most some serialisation between contexts.
hipStream_t masked_stream(int device, int ncu, int total)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, hipStream_t> pool;
    if (ncu <= 0 || ncu >= total) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto it = pool.find({device, ncu});
    if (it != pool.end()) return it->second;
    std::vector<uint32_t> mask((total + 31) / 32, 0u);
    for (int i = 0; i < total; ++i)
        if ((long)(i + 1) * ncu / total != (long)i * ncu / total) mask[i / 32] |= 1u << (i % 32);
    hipStream_t st = nullptr;
    if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); st = nullptr; }
    pool[{device, ncu}] = st;
    return st;
}

// ---- row map -------------------------------------------------------------------------------
// The N-wide products of a fraction may skip its dummy frames (GemmNT::rowmap): the map was built behind the re-layout of the
// fraction that is current now (launch_fraction_load / launch_rowmap)
// (of the axis the layer's rows lie in)
static void use_rowmap(const cn_layer *l, GemmNT &g)
{
    const TimeAxis *ax = l->ax;
    if (opt().no_nt_rowmap || !ax->pat_raw || !l->ctx->loaded) return;
    int *rm = ax->rowmap();
    g.rowcnt = rm; g.rowmap = rm + 4; g.dummymap = rm + 4 + ax->pat_maxN; g.m_est = ax->est_real;
}

// ---- timing ---------------------------------------------------------------------------------
hipEvent_t get_event(cn_ctx *c)
{
    if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
    hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return e;
}
struct Timed {
    cn_ctx *c; int cls; hipEvent_t a = nullptr; hipStream_t st;
    Timed(cn_ctx *ctx, int k, hipStream_t stream = nullptr) : c(ctx), cls(k), st(stream ? stream : ctx->stream)
    {
        if (c->timing) { a = get_event(c); hipEventRecord(a, st); }
    }
    ~Timed()
    {
        if (a) { hipEvent_t b = get_event(c); hipEventRecord(b, st); c->spans[cls].push_back({a, b}); }
    }
};

// wide softmax rows of the bf16 throughput mode: v_exp_f32 + one reciprocal per row (cn_elementwise.hip, softmax_exp<FAST>)
bool softmax_fast(cn_ctx *c)
{
    const bool exact = opt().softmax_exact;      // A/B switch
    return c->prec == P_BF16 && !exact;
}
// fp32 outputs of a feed-forward / softmax layer for a reader other than the fused softmax backward kernel
float *posteriors(cn_layer *o)
{
    cn_ctx *c = o->ctx;
    o->sm_read = true;
    if (o->sm_lazy) {
        launch_softmax_normalise(c->stream, softmax_fast(c), o->out_f32, o->ax->pat, o->ax->N, o->size, o->Lp, o->sm_stat);
        o->sm_lazy = false;
    }
    return o->out_f32;
}

// the main stream waits for everything the side stream still has in flight
void join_side(cn_ctx *c)
{
    // events of one stream complete in order: waiting for the newest of each stream covers the older ones (a wait on an
    // event that has long completed still costs the stream ~3 us, and these sit in front of the weight update)
    for (size_t i = 0; i < c->pending_joins.size(); ++i) {
        bool newest = true;
        for (size_t j = i + 1; j < c->pending_joins.size(); ++j) newest = newest && c->pending_join_streams[j] != c->pending_join_streams[i];
        if (newest) HIP_CHECK(hipStreamWaitEvent(c->stream, c->pending_joins[i], 0));
    }
    c->pending_joins.clear(); c->pending_join_streams.clear();
    // ... and for the gradient all-reduces of the communication stream (in order on that stream: the newest covers all)
    if (c->comm_pending) { HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_comm, 0)); c->comm_pending = false; }
}
// `st` waits for the gradient work of `layer` and for nothing else the context has enqueued since
void stream_wait_layer(cn_layer *layer, hipStream_t st)
{
    cn_ctx *c = layer->ctx;
    bool pending = false;
    for (hipEvent_t e : c->pending_joins) pending = pending || e == layer->ev_join;
    if (pending) { HIP_CHECK(hipStreamWaitEvent(st, layer->ev_join, 0)); return; }
    // nothing of this layer is on the side stream (CN_NO_OVERLAP, the first trainable layer, or already joined): its
    // gradient is ordered on the context's stream
    if (!c->ev_ext) HIP_CHECK(hipEventCreateWithFlags(&c->ev_ext, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(c->ev_ext, c->stream));
    HIP_CHECK(hipStreamWaitEvent(st, c->ev_ext, 0));
}

// ---- RCCL, opened at run time ----------------------------------------------------------------
// No link-time dependency: a host that never trains data-parallel needs no librccl, and a process that already holds
// one (PyTorch ships a librccl.so with the SONAME librccl.so.1) shares it instead of loading a second copy.
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
};
Rccl &rccl()
{
    static Rccl r;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (r.handle) return r;
    const char *names[] = {getenv("CN_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    std::string tried;
    for (const char *n : names) {
        if (!n || !*n) continue;
        h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
        tried += std::string(tried.empty() ? "" : "; ") + dlerror();
    }
    if (!h) throw cn_error(CN_ERR_COMM, "cannot open librccl (data-parallel training needs RCCL): " + tried);
    auto sym = [&](const char *name) {
        void *f = dlsym(h, name);
        if (!f) throw cn_error(CN_ERR_COMM, std::string("librccl lacks ") + name);
        return f;
    };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.handle = h;
    return r;
}
void rccl_check(ncclResult_t e, const char *what)
{
    if (e != ncclSuccess) throw cn_error(CN_ERR_COMM, std::string(what) + ": " + rccl().GetErrorString(e));
}
#define RCCL_CHECK(x) rccl_check((x), #x)
void require_comm(cn_ctx *c, const char *who)
{
    if (!c->has_comm()) throw cn_error(CN_ERR_STATE, std::string(who) + ": no communicator bound to this context (call cn_comm_init first)");
}
// ---- re-layout of a fraction ---------------------------------------------------------------------
bool is_class_post(const cn_layer *post)
{
    return post && (post->kind == CN_LAYER_MULTICLASS_CLASSIFICATION || post->kind == CN_LAYER_BINARY_CLASSIFICATION);
}
// the buffers a fraction is re-laid out into: the current ones, or the alternates of a prefetch
struct FractionBuffers { char *pat, *pat_raw; int *tcls; void *in_op; float *targets; };
// `f` with DEVICE pointers (the caller's resident arrays or a staging area): [T][PS] -> [T][PSp] operands, pattern types with their
// row map, classes or targets; a binary classification layer's classes become its targets
// ... augmented on the way when `aug` is on (section Input augmentation): the slot table `aug_tab` first, on the same stream
bool aug_enabled(const cn_input_augment &a) { return a.noise_sigma > 0.f || a.freq_masks > 0 || a.time_masks > 0; }
bool same_augment(const cn_input_augment &a, const cn_input_augment &b)
{
    return a.noise_sigma == b.noise_sigma && a.context_left == b.context_left && a.context_right == b.context_right &&
           a.freq_masks == b.freq_masks && a.freq_width == b.freq_width && a.time_masks == b.time_masks && a.time_width == b.time_width &&
           a.time_max_permille == b.time_max_permille && a.seed == b.seed && a.pass == b.pass;
}
bool splice_enabled(const cn_input_splice &s) { return s.frame_skip >= 1; }
bool same_splice(const cn_input_splice &a, const cn_input_splice &b)
{
    return a.context_left == b.context_left && a.context_right == b.context_right && a.frame_skip == b.frame_skip;
}
int ceil_div(int a, int b) { return (a + b - 1) / b; }
// the fraction every layer behind the re-layout sees: `f` itself, or with splicing on the network-rate lengths of the source-rate `f`
cn_fraction network_rate(const cn_input_splice &s, const cn_fraction &f)
{
    cn_fraction n = f;
    if (splice_enabled(s)) { n.max_seq_length = ceil_div(f.max_seq_length, s.frame_skip); n.min_seq_length = ceil_div(f.min_seq_length, s.frame_skip); }
    return n;
}
void check_augment_shape(const cn_input_augment &a, const cn_input_splice &sp, const cn_layer *input)
{
    if (!aug_enabled(a)) return;
    if (splice_enabled(sp) && (a.context_left != sp.context_left || a.context_right != sp.context_right))
        throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: the input augmentation's context of (" + std::to_string(a.context_left) + ", " +
                       std::to_string(a.context_right) + ") differs from the input splicing's (" + std::to_string(sp.context_left) + ", " +
                       std::to_string(sp.context_right) + ")");
    const long B = (long)a.context_left + a.context_right + 1;
    if (input->size % B != 0)
        throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: input layer size of " + std::to_string(input->size) + " is no multiple of the " +
                       std::to_string(B) + " frames of the input augmentation's context");
}
AugArgs aug_args(const cn_input_augment &a, const cn_layer *input)
{
    AugArgs g{};
    g.P0 = input->size / (a.context_left + a.context_right + 1); g.ctx_left = a.context_left;
    g.nfreq = a.freq_masks; g.fwidth = a.freq_width; g.ntime = a.time_masks; g.twidth = a.time_width; g.permille = a.time_max_permille;
    g.k0 = (uint32_t)a.seed; g.k1_noise = (uint32_t)(a.seed >> 32) ^ 0x696E7074u; g.k1_mask = (uint32_t)(a.seed >> 32) ^ 0x6D61736Bu;
    g.pass_lo = (uint32_t)a.pass; g.pass_hi = (uint32_t)(a.pass >> 32);
    g.sigma = a.noise_sigma;
    g.skip = 1;
    return g;
}
// ... of a spliced load: the augmentation's settings when it is on (its context equals the splice's: check_augment_shape), the
// geometry of the gather either way
AugArgs splice_args(const cn_input_splice &sp, const cn_input_augment &a, const cn_layer *input)
{
    AugArgs g{};
    if (aug_enabled(a)) g = aug_args(a, input);
    g.P0 = input->size / (sp.context_left + sp.context_right + 1); g.ctx_left = sp.context_left; g.skip = sp.frame_skip;
    return g;
}
void ensure_aug_table(cn_ctx *c, int *&tab)
{
    if (!tab && c->PS > 0) HIP_CHECK(hipMalloc((void **)&tab, (size_t)c->PS * AUG_TAB_STRIDE * sizeof(int)));
}
// ... gathered from a source-rate fraction when `sp` is on (section Input splicing and frame skipping): the same table first
void relayout(hipStream_t st, cn_ctx *c, cn_layer *input, cn_layer *post, const cn_fraction &f, const FractionBuffers &b,
              const cn_input_augment &aug, const cn_input_splice &sp, int *&aug_tab)
{
    const bool cls = is_class_post(post);
    const int Tnet = network_rate(sp, f).max_seq_length;
    if (splice_enabled(sp)) {
        ensure_aug_table(c, aug_tab);
        const AugArgs g = splice_args(sp, aug, input);
        launch_augment_table(st, g, f.pat_types, c->PS, f.max_seq_length, c->PS, aug_tab);
        launch_fraction_load_splice(st, c->f32, g, aug_enabled(aug), aug_tab, Tnet, c->PS, c->PSp, b.pat,
                                    cls ? f.target_classes : nullptr, b.tcls,
                                    (post && !cls) ? f.targets : nullptr, post ? b.targets : nullptr,
                                    post ? post->size : 0, f.inputs, input->size, b.in_op, input->Lp, c->rowmap_of(b.pat_raw), (int)c->pat_maxN,
                                    network_rate(sp, f).min_seq_length);
    } else if (aug_enabled(aug)) {
        ensure_aug_table(c, aug_tab);
        const AugArgs g = aug_args(aug, input);
        launch_augment_table(st, g, f.pat_types, c->PS, f.max_seq_length, c->PS, aug_tab);
        launch_fraction_load_augment(st, c->f32, g, aug_tab, f.max_seq_length, c->PS, c->PSp, f.pat_types, b.pat,
                                     cls ? f.target_classes : nullptr, b.tcls,
                                     (post && !cls) ? f.targets : nullptr, post ? b.targets : nullptr,
                                     post ? post->size : 0, f.inputs, input->size, b.in_op, input->Lp, c->rowmap_of(b.pat_raw), (int)c->pat_maxN, f.min_seq_length);
    } else {
        launch_fraction_load(st, c->f32, f.max_seq_length, c->PS, c->PSp, f.pat_types, b.pat,
                             cls ? f.target_classes : nullptr, b.tcls,
                             (post && !cls) ? f.targets : nullptr, post ? b.targets : nullptr,
                             post ? post->size : 0, f.inputs, input->size, b.in_op, input->Lp, c->rowmap_of(b.pat_raw), (int)c->pat_maxN, f.min_seq_length);
    }
    if (post && post->kind == CN_LAYER_BINARY_CLASSIFICATION)
        launch_classes_to_targets(st, b.tcls, b.targets, Tnet * c->PSp);
}
// ... out of staging area `slot`: behind its upload (copy stream); the area is free again when the re-layout has read it
void relayout_staged(hipStream_t st, cn_ctx *c, cn_layer *input, cn_layer *post, const cn_fraction &f, const FractionBuffers &b, int slot,
                     const cn_input_augment &aug, const cn_input_splice &sp, int *&aug_tab)
{
    HIP_CHECK(hipStreamWaitEvent(st, c->ev_up[slot], 0));
    relayout(st, c, input, post, f, b, aug, sp, aug_tab);
    HIP_CHECK(hipEventRecord(c->ev_free[slot], st));
    c->stage_used[slot] = true;
}
// cn_fraction_prefetch_resident / cn_fraction_prefetch: the re-layout of the announced fraction, into the alternate buffers
void launch_prefetch(cn_ctx *c, hipStream_t st)
{
    cn_ctx::Prefetch &p = c->pf;
    const FractionBuffers alt{p.pat, p.pat_raw, p.tcls, p.in_op, p.targets};
    if (p.host) relayout_staged(st, c, p.input, p.post, p.f, alt, p.slot, p.aug, p.splice, p.aug_tab);     // (f points into the staging area)
    else relayout(st, c, p.input, p.post, p.f, alt, p.aug, p.splice, p.aug_tab);
    p.launched = true;
}
// Does a backward pass hand `p` an error: is there a K8 that writes p's outputErrors, and somebody who reads them?  A trainable
// layer; or a context layer whose own predecessor does (it folds what it receives into that layer's outputErrors).  The input
// layer and a context layer behind it take none.
bool takes_err(const cn_layer *p) { return p->trainable || (p->context && takes_err(p->prev)); }

void ensure_fork_events(cn_layer *l)
{
    if (l->ev_fork) return;
    HIP_CHECK(hipEventCreateWithFlags(&l->ev_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&l->ev_join, hipEventDisableTiming));
}
// run `f(stream)` on the side stream after everything enqueued on the main stream so far
// (fork_attached: ev_fork already completes with the last main-stream kernel, see fork_event)
template <typename F> void on_side(cn_layer *l, F &&f, bool fork_attached = false)
{
    cn_ctx *c = l->ctx;
    c->tn_cus = 0;
    if (!c->overlap) { f(c->stream, nullptr); return; }
    // The first trainable layer's gradient work has nothing to run beside: only the weight update follows.  On the main
    // stream it saves the two cross-stream hand-offs (fork, join) in front of the update.
    const bool tail_on_main = !opt().tail_on_side;
    if (tail_on_main && l->prev && !takes_err(l->prev) && !fork_attached) { f(c->stream, nullptr); return; }
    ensure_fork_events(l);
    if (!fork_attached) HIP_CHECK(hipEventRecord(l->ev_fork, c->stream));
    // a recurrent kernel follows on the main stream when the preceding layer is an LSTM layer: slow lane (a CU-masked stream, so
    // that the gradient products leave the latency-bound recurrent kernel's CUs and memory path alone) -- unless the products
    // would outlast that kernel on the masked CUs and end up in front of the next N-wide product of the critical path
    // (LVCSR config: the softmax layer's 8000 x 1024 gradient took 2.0 ms on 80 CUs beside a 1.3 ms recurrent kernel and the
    // error product behind it 757 instead of 140 us; 13.3 -> 12.7 ms per fraction with the rule below)
    bool slow = c->side_slow && l->prev && l->prev->lstm;
    const bool side_rule = !opt().no_side_rule;
    // ~1.5 TFLOP/s per CU on the 64 x 64 tiles; the 256 x 256 kernel of the wide layers (cn_gemm_tn_big.hip) runs at ~3
    const TimeAxis *ax = l->ax;
    const bool big = c->prec == P_BF16 && ax->N >= 4096 && (l->lstm ? l->Hp >= 256 && l->Pp >= 192 : l->Lp >= 512 && l->Pp >= 192);
    // CUs the recurrent kernel that follows on the main stream will occupy when it is a cluster launch (0: one-CU kernels)
    int rec_cus = 0;
    if (l->prev && l->prev->lstm) {
        LstmRec r{};
        r.Hp = l->prev->Hp; r.dirs = l->prev->dirs; r.PS = c->PSp; r.T = ax->T; r.rpl = c->rpl; r.num_cus = r.cluster_cus = c->num_cus;
        rec_cus = c->d_xch ? lstm_cluster_bwd_cus(c->prec, r) : 0;
    }
    if (slow && side_rule) {
        const double flops = 2.0 * ax->N * (l->lstm ? (double)l->dirs * 4 * l->Hp * (l->Pp + l->Hp) : (double)l->Lp * l->Pp);
        const double t_side = flops / (c->side_cus * (big ? 3.0e12 : 1.5e12));
        const double t_rec = ax->T * (l->prev->Hp > 192 ? 1.2e-6 : 0.5e-6);                           // cluster / single-CU step
        if (t_side > 0.8 * t_rec) slow = false;
        // a cluster grid that covers a large part of the chip (two sequences per two-CU cluster: 112-128 CUs, each claiming its
        // CU's whole LDS) lands on the masked CUs too and leaves the masked stream a fraction of them: no slow lane then
        // (LVCSR with the masked stream beside a 128-CU grid: gradient products 10.4 -> 19.2 ms per six fractions)
        if (rec_cus > c->num_cus / 4) slow = false;
    }
    hipStream_t st = slow ? c->side_slow : c->side;
    // The 256 x 256 gradient kernel puts ONE long-lived workgroup on a CU (128 KB of LDS): beside a recurrent kernel it must leave
    // that kernel's CUs alone -- a cluster grid starts when ALL its workgroups are resident, and the recurrent workgroups claim a
    // whole CU's LDS.  Masked stream: its CUs; unmasked beside a recurrent kernel: the chip less that kernel's grid (at least 64
    // CUs: the one-CU kernels at PS = 50 / 64 take 52 - 64).  (reading B with the kernel filling the chip: 2.79 -> 2.83 ms per
    // fraction, the recurrent kernel waited.)
    c->tn_cus = slow ? c->side_cus : (l->prev && l->prev->lstm && c->num_cus > 128 ? std::max(64, c->num_cus - std::max(64, rec_cus + 8)) : 0);
    HIP_CHECK(hipStreamWaitEvent(st, l->ev_fork, 0));
    if (c->pf.valid && !c->pf.launched) launch_prefetch(c, st);      // covered by this layer's join event (same stream, in order)
    // the join event rides on the last kernel of the side work too (f returns true when it attached it)
    const bool join_attached = f(st, (c->attach_forks && !c->timing) ? l->ev_join : nullptr);
    if (!join_attached) HIP_CHECK(hipEventRecord(l->ev_join, st));
    c->pending_joins.push_back(l->ev_join); c->pending_join_streams.push_back(st);
}
// The event the side stream forks from, to be attached to the last main-stream kernel in front of the fork (a stop
// event of that launch, hipExtLaunchKernelGGL): a separate hipEventRecord is a marker packet between two kernels of the
// critical path and delays the second one by ~7 us (three to four forks per training step; 1.41 -> 1.39 ms per step with
// the fork, join and update events all riding on kernels).  nullptr: record the event the ordinary way.
hipEvent_t fork_event(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    if (!c->overlap || !c->attach_forks) return nullptr;
    ensure_fork_events(l);
    return l->ev_fork;
}
void timing_collect(cn_ctx *c)
{
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->side) HIP_CHECK(hipStreamSynchronize(c->side));
    if (c->side_slow) HIP_CHECK(hipStreamSynchronize(c->side_slow));
    if (c->comm_stream) HIP_CHECK(hipStreamSynchronize(c->comm_stream));
    for (int k = 0; k < KC_COUNT; ++k) {
        for (auto &sp : c->spans[k]) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, sp.a, sp.b));
            c->acc_ms[k] += ms; c->acc_n[k] += 1;
            c->free_events.push_back(sp.a); c->free_events.push_back(sp.b);
        }
        c->spans[k].clear();
    }
}

// ---- geometry -------------------------------------------------------------------------------
int pad_units(int H) { return H > 512 ? round_up(H, 64) : round_up(H, 32); }

// the map of a layer's own output rows (cn_unit_map.h); a follower's P and Pp are its L and Lp (cn_layer_create*)
UnitMap unit_map(const cn_layer *l)
{
    return UnitMap{l->size, l->Lp, l->lstm ? l->H : 0, l->lstm ? l->Hp : 0, l->lstm ? l->dirs : 0};
}
// does every unit have the same column in both maps (of the same L units)?  Only two directions split a row.
bool same_columns(const UnitMap &a, const UnitMap &b)
{
    const bool sa = a.H && a.dirs == 2, sb = b.H && b.dirs == 2;
    return sa == sb && (!sa || a.Hp == b.Hp);
}
LstmGeom lstm_geom(const cn_layer *l) { return LstmGeom{l->size, l->H, l->Hp, l->dirs, unit_map(l->prev)}; }
FfGeom ff_geom(const cn_layer *l) { return FfGeom{l->size, l->Lp, unit_map(l->prev)}; }
// Read-back of a layer's rows: `frames` host rows (PS slots per time step, PSp on the device) of map m at src, unpadded into the
// reference layout [frames][m.L] and copied to `host`; the stream is synchronised
void read_rows(cn_ctx *c, const void *src, bool src_is_bf16, const UnitMap &m, int frames, int PS, int PSp, float *host)
{
    const size_t bytes = (size_t)frames * m.L * sizeof(float);
    const Scratch scratch(bytes);
    float *tmp = scratch.get();
    if (m.H)
        for (int d = 0; d < m.dirs; ++d) launch_unpad(c->stream, src_is_bf16, src, m.Lp, d * m.Hp, 1, frames, m.H, tmp, m.L, d * m.H, PS, PSp);
    else launch_unpad(c->stream, src_is_bf16, src, m.Lp, 0, 1, frames, m.L, tmp, m.L, 0, PS, PSp);
    HIP_CHECK(hipMemcpyAsync(host, tmp, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
int ff_act(cn_layer_kind k)
{
    switch (k) {
    case CN_LAYER_FF_TANH: return ACT_TANH;
    case CN_LAYER_FF_LOGISTIC: return ACT_LOGISTIC;
    default: return ACT_IDENTITY;
    }
}

// ---- parameter arena ------------------------------------------------------------------------
void finalize(cn_ctx *c)
{
    if (c->finalized) return;
    size_t total = 0;
    for (cn_layer *l : c->layers)
        if (l->trainable) { l->woff = total; total += (size_t)round_up(l->nw, 4); }
    c->total = total;
    if (total) {
        HIP_CHECK(hipMalloc((void **)&c->arena, 3 * total * sizeof(float)));
        HIP_CHECK(hipMemsetAsync(c->arena, 0, 3 * total * sizeof(float), c->stream));
    }
    for (cn_layer *l : c->layers) {
        if (!l->trainable) continue;
        l->w = c->arena + l->woff;
        l->wu = c->arena + total + l->woff;
        l->wd = c->arena + 2 * total + l->woff;
        if (!l->pending_w.empty()) {
            HIP_CHECK(hipMemcpyAsync(l->w, l->pending_w.data(), l->pending_w.size() * sizeof(float),
                                     hipMemcpyHostToDevice, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            l->pending_w.clear();
        }
        l->dirty = true;
    }
    c->finalized = true;
}

// ---- optimizer rule of an update launch ---------------------------------------------------------
// a layer's JSON "learningRate" (SteepestDescentOptimizer.cu:78-80) replaces the rule's
float layer_lr(const cn_layer *l, const UpdateRule &r) { return l->own_lr >= 0.f ? l->own_lr : r.lr; }
// Weight decay (include/currennt_hip.h, section Weight decay): ld of a step at rate lr, formed in double and rounded once ...
float decay_ld(float lr, float decay) { return (float)((double)lr * (double)decay); }
// ... and the runs of a layer's flat range that decay: the input weights, and the recurrent weights of an LSTM layer
DecayRanges decay_ranges(const cn_layer *l)
{
    const size_t L = (size_t)l->size, P = (size_t)l->P;
    if (!l->lstm) return DecayRanges{L * P, 0, 0};
    return DecayRanges{4 * L * P, 4 * L * (P + 1), 4 * L * (P + 1) + 4 * L * (size_t)l->H};
}
// The scalars of include/currennt_hip.h (cn_adam_update): formed in double from the float arguments, rounded once
// lr: the effective rate (layer_lr)
AdamScalars adam_scalars(const UpdateRule &r, float lr)
{
    const double b1 = r.b1, b2 = r.b2, t = (double)r.step;
    const double c2 = std::sqrt(1.0 - std::pow(b2, t)), c1 = 1.0 - std::pow(b1, t);
    AdamScalars s;
    s.b1 = r.b1; s.b2 = r.b2; s.omb1 = (float)(1.0 - b1); s.omb2 = (float)(1.0 - b2);
    s.alpha_t = (float)((double)lr * c2 / c1); s.eps_t = (float)((double)r.eps * c2);
    return s;
}
void ensure_adam_v(cn_ctx *c)
{
    finalize(c);
    if (c->adam_v || !c->total) return;
    HIP_CHECK(hipMalloc((void **)&c->adam_v, c->total * sizeof(float)));
    HIP_CHECK(hipMemsetAsync(c->adam_v, 0, c->total * sizeof(float), c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));          // (once per context: the side and communication streams use it too)
}
// LAMB's scalars (include/currennt_hip.h, section LAMB): lr stays outside the quotient
LambScalars lamb_scalars(const cn_ctx *c, const UpdateRule &r)
{
    const double b1 = r.b1, b2 = r.b2, t = (double)r.step;
    const double c2 = std::sqrt(1.0 - std::pow(b2, t)), c1 = 1.0 - std::pow(b1, t);
    LambScalars s;
    s.b1 = r.b1; s.b2 = r.b2; s.omb1 = (float)(1.0 - b1); s.omb2 = (float)(1.0 - b2);
    s.c_t = (float)(c2 / c1); s.eps_t = (float)((double)r.eps * c2);
    s.decay = r.decay; s.min_ratio = c->trust_min; s.max_ratio = c->trust_max;
    return s;
}
// the first LAMB call: the direction vector and the layers' records (ratio 1, norms 0)
void ensure_lamb(cn_ctx *c)
{
    ensure_adam_v(c);
    if (c->lamb_u || !c->total) return;
    std::vector<LambRecord> recs;
    for (cn_layer *l : c->layers)
        if (l->trainable) { l->lamb_rec = (int)recs.size(); LambRecord r{}; r.ratio = 1.0f; recs.push_back(r); }
    HIP_CHECK(hipMalloc((void **)&c->lamb_u, c->total * sizeof(float)));
    HIP_CHECK(hipMalloc((void **)&c->lamb_recs, recs.size() * sizeof(LambRecord)));
    HIP_CHECK(hipMemsetAsync(c->lamb_u, 0, c->total * sizeof(float), c->stream));
    HIP_CHECK(hipMemcpyAsync(c->lamb_recs, recs.data(), recs.size() * sizeof(LambRecord), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
int rule_family(const UpdateRule &r) { return r.lamb ? cn_ctx::FAMILY_LAMB : r.adam ? cn_ctx::FAMILY_ADAM : cn_ctx::FAMILY_SGD; }
void bind_family(cn_ctx *c, int family, const char *fn)
{
    static const char *const calls[] = {"", "steepest descent (cn_sgd_update*, cn_ctx_arm_update)", "Adam (cn_adam_update*, cn_ctx_arm_adam)",
                                        "LAMB (cn_lamb_update*, cn_ctx_arm_lamb)"};
    static const char *const names[] = {"", "steepest descent", "Adam", "LAMB"};
    if (c->family != cn_ctx::FAMILY_NONE && c->family != family)
        throw cn_error(CN_ERR_STATE, std::string(fn) + ": this context is bound to " + calls[c->family] +
                       " by its first update, and " + names[family] +
                       " would read its weightDeltas as something they are not (momentum term / first moment)");
    c->family = family;
}
void check_adam_args(const char *fn, const UpdateRule &r)
{
    if (r.step < 1) throw cn_error(CN_ERR_BAD_ARG, std::string(fn) + ": step must be >= 1 (the caller's update count)");
    if (!(r.b1 >= 0.f && r.b1 < 1.f) || !(r.b2 >= 0.f && r.b2 < 1.f)) throw cn_error(CN_ERR_BAD_ARG, std::string(fn) + ": beta1 and beta2 must lie in [0, 1)");
    if (!(r.eps > 0.f)) throw cn_error(CN_ERR_BAD_ARG, std::string(fn) + ": eps must be > 0");
}

// one layer's operand copies from its flat weights
void launch_pack(hipStream_t st, cn_layer *l)
{
    const bool f32 = l->ctx->f32;
    if (l->lstm) launch_lstm_pack(st, f32, lstm_geom(l), l->bias, l->w, l->Win, l->WinT, l->Wrec, l->WrecT, l->bias_p, l->peep_p);
    else         launch_ff_pack(st, f32, ff_geom(l), l->bias, l->w, l->Win, l->WinT, l->bias_p);
}

void repack(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    if (l->pack_pending) {       // rebuilt on the side stream after the last update (cn_sgd_update_all)
        // ONE wait, for the last copy that was rebuilt (same stream, in order: it covers every layer's); they are all
        // done long before the second trainable layer's forward pass asks, and each wait costs the stream ~3 us
        HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_pack_last, 0));
        for (cn_layer *o : c->layers) o->pack_pending = false;
    }
    if (!l->dirty) return;
    Timed tm(c, KC_OTHER);
    launch_pack(c->stream, l);
    l->dirty = false;
}

// after a stream sync: did a bounded spin of a cluster kernel give up?
void check_fault(cn_ctx *c)
{
    int f = 0;
    HIP_CHECK(hipMemcpy(&f, c->d_fault, sizeof(int), hipMemcpyDeviceToHost));
    if (f) {
        HIP_CHECK(hipMemset(c->d_fault, 0, sizeof(int)));
        throw cn_error(CN_ERR_HIP, "recurrent cluster kernel: inter-workgroup hand-off timed out (results of this pass are invalid)");
    }
}

void require_loaded(cn_ctx *c)
{
    if (!c->loaded) throw cn_error(CN_ERR_STATE, "no fraction loaded (call cn_fraction_load first)");
}

// Weight averaging: while the weights and their average are exchanged, nothing may train on, update or overwrite what the weights
// part of the arena holds (fn: the ABI function, for the message)
void refuse_swapped(const cn_ctx *c, const char *fn)
{
    if (c->avg_swapped)
        throw cn_error(CN_ERR_STATE, std::string(fn) + ": the weights and their average are swapped (cn_ctx_swap_weight_average); swap them back first");
}

// a deferred cn_loss_accumulate that did not find a backward launch to ride on: the one-workgroup reduction now
void flush_loss(cn_ctx *c)
{
    if (!c->loss_deferred) return;
    c->loss_deferred = false;
    Timed tm(c, KC_OTHER);
    launch_rowstat_reduce(c->stream, c->d_rowstat, c->rowstat_of ? c->rowstat_of->ax->N : c->N, c->d_loss_acc, false);
}

// ---- forward / backward sequences -----------------------------------------------------------
void lstm_rec_args(cn_layer *l, LstmRec &r)
{
    cn_ctx *c = l->ctx;
    r.H = l->H; r.Hp = l->Hp; r.dirs = l->dirs; r.PS = c->PSp; r.T = l->ax->T; r.Tmin = l->ax->Tmin;
    r.pat = l->ax->pat;
    r.acts = l->acts; r.cell = l->cell; r.th = l->th; r.y_op = l->out_op; r.Wrec = l->Wrec; r.peep = l->peep_p;
    r.pre16 = nullptr;
    r.err = l->err; r.delta_op = l->delta_op; r.WrecT = l->WrecT; r.dbias = l->dbias; r.dpeep = l->dpeep;
    r.bias = l->bias;
    r.rpl = c->rpl;
    r.xch = c->d_xch; r.fault = c->d_fault; r.num_cus = r.cluster_cus = c->num_cus;
    r.xch_packed = nullptr;
    // With a communicator bound, RCCL's persistent workgroups hold CUs on the communication stream while they wait for peer
    // ranks, beside the recurrent kernel of the layer below.  A cluster grid needs ALL its members resident (spin-wait
    // hand-off), so it must fit what RCCL leaves: the grid is sized against num_cus minus a margin for RCCL's channels
    // (CN_COMM_CU_MARGIN, default 32 -- RCCL's MI300-class defaults stay at or below that many workgroups per collective);
    // a grid that no longer fits takes the streaming kernels, which make no residency assumption.  The one-CU kernels (s2, s2w,
    // 4-sequence) make none either and keep the full count, so that a data-parallel run picks the kernels of a one-GPU run.
    if (c->has_comm()) {
        const int margin = (int)opt().comm_cu_margin;
        r.cluster_cus = c->num_cus - margin > 0 ? c->num_cus - margin : 1;
    }
    r.gpart = nullptr; r.gpart_slots = 0; r.det_grid = nullptr;
    if (c->d_xch) {
        const size_t off = lstm_cluster_xch_packed_offset(c->prec, l->Hp, l->dirs, c->PSp, c->rpl, c->num_cus);
        if (off) r.xch_packed = (unsigned long long *)((char *)c->d_xch + off);
    }
    r.kname = nullptr;
    // tag range of a cluster launch (cn_lstm_cluster.hip); cleared and restarted long before the 32-bit tags wrap
    if (c->d_xch && c->xch_epoch > 0xF0000000u) { HIP_CHECK(hipMemsetAsync(c->d_xch, 0, c->xch_bytes, c->stream)); c->xch_epoch = 0; }
    r.xch_epoch = c->xch_epoch;
}

// the single-CU recurrent kernels keep two operand tiles (and, backward, one byte per time step and sequence) in LDS
// deterministic mode: the layer's workspaces for stored partial sums (zeroed; owned by the layer)
void ensure_det(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    if (l->det_ws) return;
    if (l->lstm) {
        const size_t R = (size_t)l->dirs * 4 * l->Hp;
        l->det_ws = (float *)dalloc(l, (size_t)DET_MAX_SPLITS * (R * l->Pp + R * l->Hp) * sizeof(float));
        // one slot per workgroup of the backward kernel: at most one workgroup per sequence, direction and cluster member
        l->gpart_slots = l->dirs * c->PSp * 8 + 64;
        l->gpart = (float *)dalloc(l, (size_t)l->gpart_slots * 7 * l->dirs * l->Hp * sizeof(float));
    } else {
        l->det_ws = (float *)dalloc(l, (size_t)DET_MAX_SPLITS * l->Lp * l->Pp * sizeof(float));
        l->det_colpart = (float *)dalloc(l, det_colsum_part_floats(l->Lp) * sizeof(float));
    }
}

void check_rec_lds(const cn_layer *l, bool bwd)
{
    const cn_ctx *c = l->ctx;
    const size_t need = lstm_rec_lds_bytes(c->prec, bwd, l->Hp, c->rpl, l->ax->T);
    if (need > 160 * 1024)
        throw cn_error(CN_ERR_SHAPE, "LSTM layer with " + std::to_string(l->H) + " units per direction, " + std::to_string(l->ax->T) +
                       " time steps: the recurrent " + (bwd ? "backward" : "forward") + " kernel needs " + std::to_string(need / 1024) +
                       " KB of LDS per workgroup (160 KB available)" + (c->prec == P_F32 ? "; use CN_PREC_BF16 or CN_PREC_BF16X3 for layers this wide" : "") +
                       " or shorter fractions (truncate_seq)");
}

// The next item of a group: a layer's geometry and the operand copies the launch rebuilds from its flat weights
PackItem &add_pack_item(PackGroup &grp, const cn_layer *l)
{
    PackItem &it = grp.item[grp.n++];
    it.lstm = l->lstm ? 1 : 0;
    if (l->lstm) it.lg = lstm_geom(l); else it.fg = ff_geom(l);
    it.bias = l->bias; it.w = l->w; it.Win = l->Win; it.WinT = l->WinT; it.Wrec = l->Wrec; it.WrecT = l->WrecT;
    it.bias_p = l->bias_p; it.peep_p = l->peep_p;
    return it;
}
// ... and the step that rides on it, for the item added last: update mode (PackItem::update), the rule with the layer's effective
// rate; Adam: the item's second moments and the scalars all items share
// dk: the item's ld, read by the launch when the rule's decay is on
void set_pack_update(PackGroup &grp, PackAdam &ad, PackDecayArgs &dk, int mode, const UpdateRule &r, const cn_layer *l)
{
    PackItem &it = grp.item[grp.n - 1];
    it.update = mode; it.w_rw = l->w; it.wu = l->wu; it.wd = l->wd;
    it.lr = layer_lr(l, r); it.mom = r.mom;
    dk.ld[grp.n - 1] = decay_ld(it.lr, r.decay);
    if (r.adam) {
        const AdamScalars a = adam_scalars(r, it.lr);
        it.lr = a.alpha_t; it.mom = a.b1;
        ad.v[grp.n - 1] = l->ctx->adam_v + l->woff; ad.b2 = a.b2; ad.omb1 = a.omb1; ad.omb2 = a.omb2; ad.eps_t = a.eps_t;
    }
}
// One layer's weight update + operand copies as one launch of the grouped pack kernel on `st`.
// mode 1: gradient from the flat weightUpdates; mode 2: from the packed accumulators (unpack fused in, cn_elementwise.hip)
// folds (mode 2, deterministic mode; nullable): f_in, f_rec[0], f_rec[1], f_bias -- the partial sums the launch adds itself
// r: the optimizer's rule (the armed one, or the completing call's): its kind and its decay select the instantiation
void launch_layer_update(hipStream_t st, cn_layer *l, int mode, const UpdateRule &r, hipEvent_t done, const PackFold *folds = nullptr)
{
    cn_ctx *c = l->ctx;
    PackGroup grp{};
    PackAdam ad{};
    PackDecayArgs dk{};
    PackItem &it = add_pack_item(grp, l);
    set_pack_update(grp, ad, dk, mode, r, l);
    it.wu_rw = l->wu; it.g_in = l->dWin; it.g_rec = l->dWrec; it.g_bias = l->dbias; it.g_peep = l->dpeep;
    if (folds) { it.update = 3; it.f_in = folds[0]; it.f_rec[0] = folds[1]; it.f_rec[1] = folds[2]; it.f_bias = folds[3]; }
    launch_pack_group(st, c->f32, grp, done, r.adam ? &ad : nullptr, nullptr, r.decay != 0.f ? &dk : nullptr);
    l->dirty = false; l->pack_pending = false; l->updated = true; l->noisy_ready = false;
}
// armed update without a communicator: unpack + update + operand copies ride on ONE launch behind the gradient GEMMs
bool armed_fused(const cn_layer *l) { return l->ctx->armed && !l->ctx->has_comm(); }

// ---- residual connections (include/currennt_hip.h, section Residual connections) ----
// The operand a follower of `p` reads: p's operand copy, or -- when p's last forward pass summed -- its sum buffer.  (Looked up at
// every use: a prefetch swaps the input layer's out_op.)
const void *follower_operand(const cn_layer *p) { return p->summed ? p->res_sum : p->out_op; }
// behind a marked layer's own forward kernels: the sum its followers read.  The layer records that it summed and with which
// geometry; its backward pass goes by the record.
void residual_sum(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    l->summed = false;                    // (follower_operand(l->prev) below is about the PRECEDING layer; this layer's record is set last)
    if (!l->residual) return;
    const cn_layer *p = l->prev;
    ResArgs &a = l->res;
    a.N = l->ax->N; a.own = unit_map(l); a.prev = unit_map(p);
    a.same_map = same_columns(a.own, a.prev);
    Timed tm(c, KC_OTHER);
    launch_residual_fwd(c->stream, c->f32, a, l->ax->pat, l->out_op, follower_operand(p), l->res_sum);
    l->summed = true;
}
// behind K8 and mask_handed_back_error on the main stream: the skip path's term of the preceding layer's outputErrors.  `e`: this
// layer's outputErrors as its follower handed them in.
void residual_add_error(cn_layer *l, const float *e)
{
    if (!l->summed || !takes_err(l->prev)) return;
    Timed tm(l->ctx, KC_OTHER);
    launch_residual_bwd(l->ctx->stream, l->res, l->ax->pat, e, l->prev->err);
}

// ---- layer normalization of a layer's input (include/currennt_hip.h, section Layer normalization) ----
// in front of K1 (and of the dropout copy): the normalised copy of what the preceding layer's followers read.  The layer records
// that it normalised, with which eps and geometry; its backward pass goes by the record.
const void *normalized_input(cn_layer *l, const void *x)
{
    cn_ctx *c = l->ctx;
    l->normed = l->layer_norm;
    if (!l->normed) return x;
    LnArgs &a = l->ln;
    a.N = l->ax->N; a.PS = c->PS; a.PSp = c->PSp; a.prev = unit_map(l->prev); a.eps = l->ln_eps;
    Timed tm(c, KC_OTHER);
    launch_layernorm_fwd(c->stream, c->f32, a, l->ax->pat, x, l->in_norm, l->ln_rstd);
    return l->in_norm;
}
// behind K8 and mask_handed_back_error on the main stream, in front of residual_add_error: what K8 wrote is dL/d(normalised
// copy); the preceding layer's outputErrors become dL/d(its output) along the weighted path.  (K9 reads in_norm on the side
// stream meanwhile; nobody writes it.)
void normalize_handed_back_error(cn_layer *l)
{
    if (!l->normed || !takes_err(l->prev)) return;
    Timed tm(l->ctx, KC_OTHER);
    launch_layernorm_bwd(l->ctx->stream, l->ctx->f32, l->ln, l->ax->pat, l->in_norm, l->ln_rstd, l->prev->err);
}

// ---- dropout on a layer's input (include/currennt_hip.h, section Dropout) ----
// The operand a layer's input products read in this forward pass: the preceding layer's operand copy (normalised first when the
// layer is marked for it), or -- when the pass drops -- the masked copy of that, written here in front of K1.  The layer records
// whether it dropped and with which key: its backward pass (the input-weight gradient's operand, the mask of the error it hands
// back) goes by the record, not by the context's state then.
const void *forward_input(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    const void *x = normalized_input(l, follower_operand(l->prev));
    l->dropped = c->drop_enable && l->drop_rate > 0.f;
    if (!l->dropped) return x;
    DropArgs &a = l->drop;
    a.N = l->ax->N; a.PS = c->PS; a.PSp = c->PSp; a.prev = unit_map(l->prev);
    a.k0 = (uint32_t)c->drop_seed + (uint32_t)l->ordinal; a.k1 = (uint32_t)(c->drop_seed >> 32);
    a.pass_lo = (uint32_t)c->drop_pass; a.pass_hi = (uint32_t)(c->drop_pass >> 32);
    a.thr = (uint32_t)std::floor((double)l->drop_rate * 4294967296.0);
    a.scale = (float)(1.0 / (1.0 - (double)l->drop_rate));
    Timed tm(c, KC_OTHER);
    launch_dropout_fwd(c->stream, c->f32, a, x, l->in_drop);
    return l->in_drop;
}
// the same operand for the input-weight gradient of the backward pass
const void *backward_input(const cn_layer *l) { return l->dropped ? l->in_drop : l->normed ? l->in_norm : follower_operand(l->prev); }
// behind K8 on the main stream: the error handed to the preceding layer passes the forward pass's mask
void mask_handed_back_error(cn_layer *l)
{
    if (!l->dropped) return;
    Timed tm(l->ctx, KC_OTHER);
    launch_dropout_bwd(l->ctx->stream, l->drop, l->prev->err);
}

// ---- weight noise (include/currennt_hip.h, section Weight noise) ----
// The noisy set of every trainable layer whose set is stale, in ONE launch on `st`, from the triple in force and the flat weights
// as they are (the first use allocates the sets).
void generate_noisy(cn_ctx *c, hipStream_t st)
{
    {
        Timed tm(c, KC_OTHER, st);
        PackGroup grp{};
        PackNoise nz{};
        nz.k1 = (uint32_t)(c->noise_seed >> 32) ^ 0x6E6F6973u;
        nz.pass_lo = (uint32_t)c->noise_pass; nz.pass_hi = (uint32_t)(c->noise_pass >> 32);
        nz.sigma = c->noise_sigma;
        for (cn_layer *o : c->layers) {
            if (!o->trainable || o->noisy_ready) continue;
            if (!o->nWinT) {
                const size_t e = c->esz();
                if (o->lstm) {
                    const size_t R = (size_t)o->dirs * 4 * o->Hp;
                    o->nWinT = dalloc(o, R * o->Pp * e); o->nWrecT = dalloc(o, R * o->Hp * e);
                    o->npeep = (float *)dalloc(o, (size_t)o->dirs * 3 * o->Hp * sizeof(float));
                } else o->nWinT = dalloc(o, (size_t)o->Lp * o->Pp * e);
            }
            PackItem &it = add_pack_item(grp, o);
            it.Win = nullptr; it.Wrec = nullptr; it.bias_p = nullptr;
            it.WinT = o->nWinT; it.WrecT = o->nWrecT; it.peep_p = o->npeep;
            nz.k0[grp.n - 1] = (uint32_t)c->noise_seed + (uint32_t)o->ordinal;
            o->noisy_ready = true;
            if (grp.n == PACK_GROUP_MAX) { launch_pack_group_noise(st, c->f32, grp, nz); grp.n = 0; }
        }
        if (grp.n) launch_pack_group_noise(st, c->f32, grp, nz);
    }
}
// In front of a layer's backward kernels, on the main stream: does this pass read the noisy set of the layer's copies?  A stale
// set is generated here, with every other stale one: the first backward call of a pass pays for all layers.  (The noise is a
// function of the key and the flat weights, which no backward pass of the layers above changes for the layers below: an armed
// update rewrites its own layer only, and marks that layer's set stale.)
bool backward_noise(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    l->noise_used = c->noise_sigma != 0.f;
    if (!l->noise_used) return false;
    if (c->noise_wait) { HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_noise, 0)); c->noise_wait = false; }
    if (!l->noisy_ready) generate_noisy(c, c->stream);
    l->noisy_ready = false;               // consumed: the next pass of this layer has a set of its own generated
    return true;
}
// Option noise_ahead, in front of the first trainable layer's forward pass: the key of the coming backward pass is known already
// (cn_ctx_set_weight_noise precedes the pass), so the stale sets are generated on the side stream beside the forward pass.  The
// side stream forks from the main stream here: behind the last update of the weights and the last backward kernels that read
// the sets.  A triple or weights that change before the backward pass make the sets stale again, and backward_noise generates
// them in place.
void noise_ahead(cn_ctx *c)
{
    if (c->noise_sigma == 0.f || !c->overlap || !c->side || c->timing) return;
    bool any = false;
    for (cn_layer *o : c->layers) {
        if (!o->trainable || o->noisy_ready) continue;
        if (!o->nWinT) return;            // (the first generation allocates, on the main stream)
        any = true;
    }
    if (!any) return;
    if (!c->ev_noise) {
        HIP_CHECK(hipEventCreateWithFlags(&c->ev_noise_fork, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&c->ev_noise, hipEventDisableTiming));
    }
    HIP_CHECK(hipEventRecord(c->ev_noise_fork, c->stream));
    HIP_CHECK(hipStreamWaitEvent(c->side, c->ev_noise_fork, 0));
    generate_noisy(c, c->side);
    HIP_CHECK(hipEventRecord(c->ev_noise, c->side));
    c->noise_wait = true;
}

// ---- context layers (include/currennt_hip.h, section Context layers) ----
// The slot lengths of the current fraction, formed on the device on the context's stream, once per fraction
void context_lengths(cn_ctx *c)
{
    if (c->cx_serial == c->frac_serial) return;
    launch_context_lengths(c->stream, c->d_pat, c->T, c->PSp, c->cx_len);
    c->cx_serial = c->frac_serial;
}
// ---- the time axis of a layer (include/currennt_hip.h, section Strided context layers) ----
// A call in an axis that its strided layer has not formed for the current fraction has no steps, pattern types or classes to go by
void require_axis(const cn_layer *l, const char *fn)
{
    const TimeAxis *ax = l->ax;
    if (ax->owner && ax->serial != l->ctx->frac_serial)
        throw cn_error(CN_ERR_STATE, std::string(fn) + ": the strided context layer in front of this layer has no forward pass of the current fraction");
}
// the slot lengths of the axis a context layer READS (its predecessor's): the base axis forms them on demand
const int *parent_lengths(cn_layer *l, const char *fn)
{
    cn_ctx *c = l->ctx;
    require_axis(l->prev, fn);
    if (!l->prev->ax->owner) { context_lengths(c); return c->cx_len; }
    return l->prev->ax->len;
}
// A strided layer's own axis, once per fraction, in front of its gather: steps by host arithmetic; lengths, pattern types and
// classes by one kernel over all T' * PSp rows; then the row map with Tmin' steps of unchecked rows
void form_axis(cn_layer *l, const int *plen)
{
    cn_ctx *c = l->ctx;
    TimeAxis &ax = l->own_axis;
    if (ax.serial == c->frac_serial) return;
    const TimeAxis &pa = *l->prev->ax;
    const int S = l->cx_stride;
    ax.T = ceil_div(pa.T, S); ax.Tmin = ceil_div(pa.Tmin, S); ax.N = ax.T * c->PSp; ax.Next = ax.T * c->PS;
    ax.est_real = c->numSeqs * ((ax.Tmin + ax.T + 1) / 2);
    launch_stride_axis(c->stream, S, ax.T, c->PSp, plen, pa.tcls, ax.len, ax.pat, ax.tcls);
    launch_rowmap(c->stream, ax.pat, ax.N, ax.rowmap(), (int)ax.pat_maxN, ax.Tmin * c->PSp);
    ax.serial = c->frac_serial;
}
// the target rows a post output layer compares with: the loads' own, or behind a strided layer the rows of its axis
// (every caller -- the post layer's backward pass, cn_loss_eval, cn_loss_accumulate -- holds a Timed scope of KC_OTHER around it)
const float *post_targets(cn_layer *post)
{
    cn_ctx *c = post->ctx;
    const TimeAxis *ax = post->ax;
    if (!ax->owner || !post->targets) return post->targets;
    if (post->ax_targets_serial != c->frac_serial) {
        launch_stride_targets(c->stream, ax->rate, ax->T, c->PSp, post->size, ax->len, post->targets, post->ax_targets);
        post->ax_targets_serial = c->frac_serial;
    }
    return post->ax_targets;
}
void context_forward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    const cn_layer *p = l->prev;
    Timed tm(c, KC_OTHER);
    const int *len = parent_lengths(l, "cn_layer_forward");
    ContextArgs &a = l->cx;
    a.Tin = p->ax->T; a.Tout = ceil_div(p->ax->T, l->cx_stride); a.PSp = c->PSp; a.B = l->cx_left + l->cx_right + 1;
    a.left = l->cx_left; a.dil = l->cx_dil; a.Lp = l->Lp; a.S = l->cx_stride;
    a.prev = unit_map(p);
    if (l->cx_stride > 1) form_axis(l, len);
    launch_context_fwd(c->stream, c->f32, a, len, follower_operand(p), l->out_op);
}
// behind the follower's K8 (and its mask / normalisation / skip term) on the main stream: the preceding layer's outputErrors.
// Nothing to do when that layer takes none -- the follower then had no K8 either.
void context_backward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    if (!takes_err(l->prev)) return;
    // (a plain layer lies in its predecessor's axis: l->ax->T == l->prev->ax->T there)
    if (l->cx.Tin != l->prev->ax->T || l->cx.PSp != c->PSp || (l->cx_stride > 1 && l->own_axis.serial != c->frac_serial))
        throw cn_error(CN_ERR_STATE, "cn_layer_backward: the context layer has no forward pass of the current fraction");
    Timed tm(c, KC_OTHER);
    launch_context_bwd(c->stream, l->cx, parent_lengths(l, "cn_layer_backward"), l->err, l->prev->err);
}

void lstm_forward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    const int R = l->dirs * 4 * l->Hp;
    repack(l);
    const void *x = forward_input(l);
    // bf16 mode, two-sequence forward kernels: the pre-activations leave the product as bf16 (8 instead of 16 bytes per unit and
    // frame -- the product is bound by that store: 72 of the 88 MB a headline launch moved) and the recurrent kernel widens them
    bool pre16 = false;
    if (l->pre16) {
        LstmRec probe; lstm_rec_args(l, probe);
        pre16 = lstm_cluster_size(c->prec, l->Hp, l->dirs, c->PSp, c->rpl, probe.cluster_cus) == 0 && lstm_fwd_takes_pre16(c->prec, probe);
    }
    {   // K1: gate pre-activations of all frames, 4 gates x dirs packed into one N = R product
        Timed tm(c, KC_GEMM_WIDE);
        GemmNT g{};
        g.A = x; g.lda = l->Pp; g.B = l->Win; g.ldb = l->Pp;
        g.C = l->acts; g.ldc = R; g.C2 = nullptr; g.ldc2 = 0; g.bias = l->bias_p; g.act = ACT_IDENTITY;
        if (pre16) { g.C = nullptr; g.C2 = l->pre16; g.ldc2 = R; }
        g.M = l->ax->N; g.N = R; g.K = l->Pp;
        if (l->prev->lstm) use_rowmap(l, g);          // (y = 0 on dummy frames; what the caller's inputs hold there is the caller's business)
        launch_gemm_nt(c->stream, c->prec, g);
    }
    {   // K2+K3+K4: the whole time loop
        Timed tm(c, KC_REC_FWD);
        LstmRec r; lstm_rec_args(l, r); r.kname = l->kname[0];
        if (pre16) r.pre16 = l->pre16;
        if (!launch_lstm_cluster(c->stream, c->prec, false, r, &c->xch_epoch)) { check_rec_lds(l, false); launch_lstm_forward(c->stream, c->prec, r); }
        HIP_CHECK(hipGetLastError());
    }
    residual_sum(l);
}

void lstm_backward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    const int R = l->dirs * 4 * l->Hp, Hp = l->Hp, PS = c->PSp, N = l->ax->N;
    const size_t e = c->esz();
    repack(l);
    const bool noisy = backward_noise(l);   // every backward product with a weight in it then reads the noisy set: WrecT, peep, WinT
    bool fork_attached = false;
    // (the packed gradient accumulators are zero here: allocation clears them, the unpack kernel re-clears them)
    int det_grid = 0;
    if (c->det) ensure_det(l);
    {   // K5+K6+K7 and the bias / peephole sums of K9
        Timed tm(c, KC_REC_BWD);
        LstmRec r; lstm_rec_args(l, r); r.kname = l->kname[1];
        if (noisy) { r.WrecT = l->nWrecT; r.peep = l->npeep; }
        if (c->det) { r.gpart = l->gpart; r.gpart_slots = l->gpart_slots; r.det_grid = &det_grid; }
        if (!launch_lstm_cluster(c->stream, c->prec, true, r, &c->xch_epoch)) {
            check_rec_lds(l, true);
            // no K8 behind this kernel (the preceding layer is the input layer): the side stream forks from it directly
            const bool tail_on_side = opt().tail_on_side;
            hipEvent_t fork = (tail_on_side && !takes_err(l->prev) && !c->timing) ? fork_event(l) : nullptr;
            launch_lstm_backward(c->stream, c->prec, r, fork);
            fork_attached = fork != nullptr;
        }
        HIP_CHECK(hipGetLastError());
    }
    if (takes_err(l->prev)) {   // K8 (LstmLayer.cu:990-1009): one K = R product instead of 4*dirs
        Timed tm(c, KC_GEMM_WIDE);
        GemmNT g{};
        g.A = l->delta_op; g.lda = R; g.B = noisy ? l->nWinT : l->WinT; g.ldb = R;
        g.C = l->prev->err; g.ldc = l->prev->Lp; g.bias = nullptr; g.act = ACT_IDENTITY;
        g.M = N; g.N = l->Pp; g.K = R;
        use_rowmap(l, g);
        hipEvent_t fork = c->timing ? nullptr : fork_event(l);     // (timing mode records its own events around the kernel)
        launch_gemm_nt(c->stream, c->prec, g, fork);
        fork_attached = fork != nullptr;
    }
    if (takes_err(l->prev)) mask_handed_back_error(l);    // (K8 carries the fork: K9 does not read prev->err and starts beside this)
    normalize_handed_back_error(l);
    residual_add_error(l, l->err);        // (the recurrent kernels only read l->err: LstmRec::err is const, the hand-written loops only load from it)
    // K9 runs on the side stream: it only feeds weightUpdates, forked AFTER K8 so the critical-path GEMM has the chip to itself, and running beside the
    // preceding layer's recurrent kernel (which occupies ~10 % of the CUs)
    on_side(l, [&](hipStream_t st, hipEvent_t join) {
        // deterministic mode with the armed, fused update behind the products: that launch adds the partial sums itself (no fold
        // launch at all); otherwise one fold launch rides behind the grouped product
        const bool fused = armed_fused(l);
        const bool defer = c->det && fused;
        int used_in = 0, used_rec[2] = {0, 0};
        {   // K9 input weights: dWin[r][i] = sum_n delta[n][r] x[n][i]
            Timed tm(c, KC_GEMM_GRAD, st);
            GemmTN gs[3]; int ng = 0;
            GemmTN g{};
            g.A = l->delta_op; g.lda = R; g.B = backward_input(l); g.ldb = l->Pp;
            g.C = l->dWin; g.ldc = l->Pp; g.M = R; g.N = l->Pp; g.K = N;
            if (c->det) { g.ws = l->det_ws; g.ws_splits = DET_MAX_SPLITS; g.ws_used = defer ? &used_in : nullptr; }
            gs[ng++] = g;
            // K9 recurrent weights: dWrec[(j,g)][i] = sum_t delta[t][(j,g)] y[prev(t)][i]
            if (N > PS) {
                for (int d = 0; d < l->dirs; ++d) {
                    GemmTN r{};
                    const char *dl = (const char *)l->delta_op + (size_t)d * 4 * Hp * e;
                    const char *y = (const char *)l->out_op + (size_t)d * Hp * e;
                    if (d == 0) { r.A = dl + (size_t)PS * R * e; r.B = y; }                       // skipFirstPattern, LstmLayer.cu:432-435
                    else        { r.A = dl; r.B = y + (size_t)PS * l->Lp * e; }                   // skipLastPattern,  :428-431
                    r.lda = R; r.ldb = l->Lp;
                    r.C = l->dWrec + (size_t)d * 4 * Hp * Hp; r.ldc = Hp; r.M = 4 * Hp; r.N = Hp; r.K = N - PS;
                    if (c->det) { r.ws = l->det_ws + (size_t)DET_MAX_SPLITS * ((size_t)R * l->Pp + (size_t)d * 4 * Hp * Hp); r.ws_splits = DET_MAX_SPLITS; r.ws_used = defer ? &used_rec[d] : nullptr; }
                    gs[ng++] = r;
                }
            }
            // deterministic mode: the workgroups' bias / peephole sums, added in workgroup order (dbias and dpeep are neighbours, in
            // the gradient block and in a slot alike), in the launch that adds the products' split partials
            const int slot = 7 * l->dirs * Hp;
            const FoldItem f{l->dbias, l->gpart, (long)slot, det_grid, 1, slot, slot, 1, 1};
            launch_gemm_tn_group(st, c->prec, gs, ng, c->tn_cus, (c->det && !defer) ? &f : nullptr);      // the three products side by side in one launch
        }
        {
            Timed tm(c, KC_OTHER, st);
            if (fused) {
                const int slot = 7 * l->dirs * Hp;
                const PackFold folds[4] = {
                    {l->det_ws, (long)R * l->Pp, used_in, 0},
                    {l->det_ws ? l->det_ws + (size_t)DET_MAX_SPLITS * (size_t)R * l->Pp : nullptr, 4L * Hp * Hp, used_rec[0], 0},
                    {l->det_ws ? l->det_ws + (size_t)DET_MAX_SPLITS * ((size_t)R * l->Pp + (size_t)4 * Hp * Hp) : nullptr, 4L * Hp * Hp, used_rec[1], 0},
                    {l->gpart, (long)slot, det_grid, 1}};
                launch_layer_update(st, l, 2, c->arm, join, defer ? folds : nullptr);
            } else launch_lstm_unpack_grads(st, lstm_geom(l), l->dWin, l->dWrec, l->dbias, l->dpeep, l->wu, join);
        }
        return join != nullptr;
    }, fork_attached);
}

void ff_forward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    repack(l);
    const bool softmax = l->kind == CN_LAYER_SOFTMAX;
    const void *x = forward_input(l);
    {
        Timed tm(c, KC_GEMM_WIDE);
        GemmNT g{};
        g.A = x; g.lda = l->Pp; g.B = l->Win; g.ldb = l->Pp;
        g.C = l->out_f32; g.ldc = l->Lp;
        g.C2 = (!c->f32 && !softmax) ? l->out_op : nullptr; g.ldc2 = l->Lp;
        g.bias = l->bias_p; g.act = ff_act(l->kind);
        g.M = l->ax->N; g.N = l->Lp; g.K = l->Pp;
        if (l->prev->lstm) use_rowmap(l, g);          // (y = 0 on dummy frames, ComputeBlockOutputFn; a feed-forward layer's output is act(bias) there)
        launch_gemm_nt(c->stream, c->prec, g);
    }
    if (softmax) {
        for (cn_layer *p : c->layers) if (p->prev == l) p->ctc_swept = false;      // (a ctc layer's sweeps belonged to the old posteriors)
        l->fwd_serial = c->frac_serial;
        flush_loss(c);                         // (the row statistics are about to be overwritten)
        Timed tm(c, KC_OTHER);
        const bool stat = c->d_rowstat != nullptr;
        // wide rows in training: the posteriors are only ever read by the fused backward kernel, which can recompute them from the
        // logits -- 1.1 GB less to write per fraction of the 8000-class output layer.  A layer whose posteriors were asked for after
        // its last forward pass (forward-only use, another loss than multiclass) runs the eager kernel.  Only where recomputing is
        // cheap (softmax_fast): with expf and a division per element the two lazy passes take longer than the eager ones
        // (probe/softmax_bench: 363 + 633 against 454 + 427 us).
        const bool lazy_off = opt().no_lazy_softmax;
        const bool lazy_force = opt().lazy_softmax;                              // the exact lazy kernels
        l->sm_lazy = stat && l->sm_stat && l->sm_lazy_next && !l->has_follower && !lazy_off && (softmax_fast(c) || lazy_force);
        l->sm_read = false;
        launch_softmax_fwd(c->stream, l->out_f32, l->ax->pat, l->ax->N, l->size, l->Lp, stat ? l->ax->tcls : nullptr, stat ? c->d_rowstat : nullptr,
                           softmax_fast(c), l->sm_lazy ? l->sm_stat : nullptr);
        c->rowstat_of = stat ? l : nullptr;
        if (!c->f32 && l->has_follower) launch_pad_convert(c->stream, false, l->out_f32, l->ax->N, l->Lp, l->out_op, l->Lp);
    }
    residual_sum(l);
}

void ff_backward(cn_layer *l)
{
    cn_ctx *c = l->ctx;
    const int N = l->ax->N;
    repack(l);
    const bool noisy = backward_noise(l);
    if (c->det) ensure_det(l);
    FoldItem colfold{}; colfold.nparts = 0;       // deterministic mode: the column sums' fold rides on the gradient product's
    bool dummy_deltas_zero = false;               // (the row map's condition: every operand row of a dummy frame is zero)
    {
        Timed tm(c, KC_OTHER);
        if (l->kind == CN_LAYER_SOFTMAX && l->mcc_pending && l->Lp <= 8192) {
            dummy_deltas_zero = true;             // softmax_mcc_bwd_kernel stores zeros for every pattern that is not real
            // bf16 mode: the fp32 outputErrors stay unwritten (read back from the bf16 operand copy if anyone asks)
            const bool with_loss = c->loss_deferred && c->rowstat_of == l && softmax_mcc_bwd_takes_loss(l->Lp);
            launch_softmax_mcc_bwd(c->stream, c->f32, l->out_f32, l->ax->tcls, l->ax->pat, N, l->size, l->Lp, c->f32 ? l->err : nullptr, l->delta_op, l->dbias,
                                   with_loss ? c->d_rowstat : nullptr, with_loss ? c->d_loss_acc : nullptr, c->d_loss + 6, l->sm_lazy ? l->sm_stat : nullptr,
                                   softmax_fast(c), c->d_colpart, c->det ? l->det_colpart : nullptr, &colfold);
            l->sm_lazy_next = !l->sm_read;
            if (with_loss) c->loss_deferred = false;
            l->err_in_delta = !c->f32;
        } else {
            l->err_in_delta = false;
            if (l->kind == CN_LAYER_SOFTMAX) l->sm_lazy_next = false;   // no fused consumer: lazy rows would be normalised on demand every pass
            const float *y = posteriors(l);                 // (the branch: act' of a marked layer is taken at its own output, not at the sum)
            // a marked layer hands its outputErrors on as they came in: launch_ff_delta below overwrites them in place
            if (l->summed && takes_err(l->prev))
                HIP_CHECK(hipMemcpyAsync(l->res_e, l->err, (size_t)N * l->Lp * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            if (l->mcc_pending) launch_mcc_backward(c->stream, y, l->ax->tcls, N, l->size, l->Lp, l->err);
            if (l->kind == CN_LAYER_SOFTMAX) launch_softmax_bwd(c->stream, y, l->err, l->ax->pat, N, l->size, l->Lp);
            launch_ff_delta(c->stream, c->f32, ff_act(l->kind), y, l->err, l->delta_op, N, l->size, l->Lp);
            launch_colsum(c->stream, l->err, N, l->Lp, l->dbias, c->det ? l->det_colpart : nullptr, &colfold);
        }
        l->mcc_pending = false;
    }
    bool fork_attached = false;
    if (takes_err(l->prev)) {   // FeedForwardLayer.cu:188-198
        Timed tm(c, KC_GEMM_WIDE);
        GemmNT g{};
        g.A = l->delta_op; g.lda = l->Lp; g.B = noisy ? l->nWinT : l->WinT; g.ldb = l->Lp;
        g.C = l->prev->err; g.ldc = l->prev->Lp; g.bias = nullptr; g.act = ACT_IDENTITY;
        g.M = N; g.N = l->Pp; g.K = l->Lp;
        if (dummy_deltas_zero) use_rowmap(l, g);
        hipEvent_t fork = c->timing ? nullptr : fork_event(l);
        launch_gemm_nt(c->stream, c->prec, g, fork);
        fork_attached = fork != nullptr;
    }
    if (takes_err(l->prev)) mask_handed_back_error(l);
    normalize_handed_back_error(l);
    residual_add_error(l, l->res_e);
    on_side(l, [&](hipStream_t st, hipEvent_t join) {
        const bool fused = armed_fused(l);
        const bool defer = c->det && fused;
        int used_in = 0;
        {   // FeedForwardLayer.cu:200-207
            Timed tm(c, KC_GEMM_GRAD, st);
            GemmTN g{};
            g.A = l->delta_op; g.lda = l->Lp; g.B = backward_input(l); g.ldb = l->Pp;
            g.C = l->dWin; g.ldc = l->Pp; g.M = l->Lp; g.N = l->Pp; g.K = N;
            if (c->det) { g.ws = l->det_ws; g.ws_splits = DET_MAX_SPLITS; g.ws_used = defer ? &used_in : nullptr; }
            launch_gemm_tn(st, c->prec, g, c->tn_cus, (colfold.nparts && !defer) ? &colfold : nullptr);
        }
        {
            Timed tm(c, KC_OTHER, st);
            if (fused) {
                // (the column sums' partial rows: colfold describes them; its target, the packed bias gradient, stays zero)
                const PackFold folds[4] = {{l->det_ws, (long)l->Lp * l->Pp, used_in, 0}, {nullptr, 0, 0, 0}, {nullptr, 0, 0, 0},
                                           {colfold.part, colfold.stride, colfold.nparts, 0}};
                launch_layer_update(st, l, 2, c->arm, join, defer ? folds : nullptr);
            } else launch_ff_unpack_grads(st, ff_geom(l), l->bias, l->dWin, l->dbias, l->wu, join);
        }
        return join != nullptr;
    }, fork_attached);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
extern "C" {

const char *cn_version(void) { return "currennt_hip 0.1 (gfx950)"; }

const char *cn_last_error(cn_ctx *) { return g_last_error.c_str(); }

const char *cn_device_arch(cn_ctx *ctx) { return ctx ? ctx->arch.c_str() : ""; }

int cn_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return count;
}

int cn_device_name(int index, char *buf, int buf_size)
{
    if (!buf || buf_size <= 0) { g_last_error = "cn_device_name: bad buffer"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, index));
        snprintf(buf, (size_t)buf_size, "%s (%s)", prop.name, prop.gcnArchName);
    });
}

int cn_ctx_create(int device_id, cn_precision precision, void *stream, cn_ctx **out)
{
    if (!out) { g_last_error = "cn_ctx_create: out is NULL"; return CN_ERR_BAD_ARG; }
    *out = nullptr;
    if (precision != CN_PREC_F32 && precision != CN_PREC_BF16 && precision != CN_PREC_BF16X3) { g_last_error = "cn_ctx_create: unknown precision"; return CN_ERR_BAD_ARG; }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        g_last_error = "cn_ctx_create: no HIP device available (this library has no CPU fallback)";
        return CN_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= count) { g_last_error = "cn_ctx_create: device id out of range"; return CN_ERR_BAD_ARG; }
    cn_ctx *c = nullptr;
    int rc = guarded([&] {
        HIP_CHECK(hipSetDevice(device_id));
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
        std::string arch = prop.gcnArchName;
        if (arch.rfind("gfx950", 0) != 0)
            throw cn_error(CN_ERR_NO_DEVICE, "cn_ctx_create: device is " + arch + ", this library is built for gfx950 only");
        c = new cn_ctx;
        c->device = device_id; c->arch = arch; c->f32 = (precision != CN_PREC_BF16);
        c->prec = precision == CN_PREC_BF16 ? P_BF16 : (precision == CN_PREC_BF16X3 ? P_X3 : P_F32);
        c->num_cus = prop.multiProcessorCount;
        if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
        else { HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
        HIP_CHECK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        {
            // 5/16 of the CUs (80 of 256) measured best; counts that divide the CU numbering evenly (32, 64, 96) put the
            // mask on few XCDs and gain nothing.  CN_SIDE_CUS=0 turns the slow lane off.
            int ncu = prop.multiProcessorCount * 5 / 16;
            if (const char *e = getenv("CN_SIDE_CUS")) ncu = atoi(e);
            c->side_slow = masked_stream(device_id, ncu, prop.multiProcessorCount);
            c->side_cus = ncu;
        }
        c->opt = options_from_env();            // the one place the switches' environment variables are read for this context
        cn::t_opt = &c->opt;
        c->det = precision != CN_PREC_BF16;
        if (const char *e = getenv("CN_DETERMINISTIC")) c->det = atoi(e) != 0;
        if (const char *e = getenv("CN_NO_OVERLAP")) c->overlap = atoi(e) == 0;
        if (const char *e = getenv("CN_NO_ATTACHED_FORKS")) c->attach_forks = atoi(e) == 0;
        if (const char *e = getenv("CN_RPL")) c->rpl_override = atoi(e);   // experiments: force 4/8/16 sequences per workgroup
        // per call | running sums | sums over all ranks | 16 x {sum, count} partials + arrival counter of the loss sum that rides on
        // the output layer's backward launch (softmax_mcc_bwd_kernel)
        HIP_CHECK(hipMalloc((void **)&c->d_loss, (6 + 2 * 16 + 2) * sizeof(float)));
        HIP_CHECK(hipMemsetAsync(c->d_loss, 0, (6 + 2 * 16 + 2) * sizeof(float), c->stream));
        c->d_loss_acc = c->d_loss + 2;
        HIP_CHECK(hipMalloc((void **)&c->d_colpart, softmax_mcc_bwd_colpart_floats() * sizeof(float)));
        HIP_CHECK(hipMemsetAsync(c->d_colpart, 0, softmax_mcc_bwd_colpart_floats() * sizeof(float), c->stream));
        HIP_CHECK(hipMalloc((void **)&c->d_fault, sizeof(int)));
        HIP_CHECK(hipMemsetAsync(c->d_fault, 0, sizeof(int), c->stream));
    });
    if (rc != CN_OK) { delete c; return rc; }
    *out = c;
    return CN_OK;
}

int cn_ctx_destroy(cn_ctx *ctx)
{
    if (!ctx) return CN_OK;
    return guarded([&] {
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
        lstm_cluster_stream_gone(ctx->stream);
        if (ctx->side) { hipStreamSynchronize(ctx->side); hipStreamDestroy(ctx->side); }
        if (ctx->side_slow) hipStreamSynchronize(ctx->side_slow);     // shared per device, never destroyed: masked_stream()
        if (ctx->ev_sgd) hipEventDestroy(ctx->ev_sgd);
        if (ctx->ev_ext) hipEventDestroy(ctx->ev_ext);
        if (ctx->ev_noise) { hipEventDestroy(ctx->ev_noise); hipEventDestroy(ctx->ev_noise_fork); }
        if (ctx->copy) { hipStreamSynchronize(ctx->copy); hipStreamDestroy(ctx->copy); }
        if (ctx->comm_stream) hipStreamSynchronize(ctx->comm_stream);
        if (ctx->comm) { (void)rccl().CommDestroy(ctx->comm); ctx->comm = nullptr; }
        if (ctx->ipc) { ipc_comm_destroy(ctx->ipc); ctx->ipc = nullptr; }
        if (ctx->comm_stream) { hipStreamDestroy(ctx->comm_stream); hipEventDestroy(ctx->ev_comm); hipEventDestroy(ctx->ev_comm_fork); }
        for (int i = 0; i < 2; ++i) {
            if (ctx->h_stage[i]) hipHostFree(ctx->h_stage[i]);
            if (ctx->d_stage[i]) hipFree(ctx->d_stage[i]);
            if (ctx->ev_up[i]) { hipEventDestroy(ctx->ev_up[i]); hipEventDestroy(ctx->ev_free[i]); }
        }
        std::vector<cn_layer *> ls = ctx->layers;
        for (cn_layer *l : ls) {
            for (void *p : l->owned) hipFree(p);
            if (l->ev_fork) { hipEventDestroy(l->ev_fork); hipEventDestroy(l->ev_join); }
            if (l->ev_pack) hipEventDestroy(l->ev_pack);
            for (int b = 0; b < 2; ++b) if (l->ctc_hbuf[b]) { hipHostFree(l->ctc_hbuf[b]); hipEventDestroy(l->ctc_ev[b]); }
            delete l;
        }
        for (int k = 0; k < KC_COUNT; ++k) for (auto &sp : ctx->spans[k]) { hipEventDestroy(sp.a); hipEventDestroy(sp.b); }
        for (hipEvent_t e : ctx->free_events) hipEventDestroy(e);
        hipFree(ctx->pf.pat_raw); hipFree(ctx->pf.tcls); hipFree(ctx->d_colpart); hipFree(ctx->aug_tab); hipFree(ctx->pf.aug_tab);
        hipFree(ctx->d_pat_raw); hipFree(ctx->d_tcls); hipFree(ctx->d_loss); hipFree(ctx->arena); hipFree(ctx->adam_v); hipFree(ctx->lamb_u); hipFree(ctx->lamb_recs); hipFree(ctx->avg); hipFree(ctx->clip_rec); hipFree(ctx->acc); hipFree(ctx->d_rowstat); hipFree(ctx->d_xch); hipFree(ctx->d_fault); hipFree(ctx->cx_len); hipFree(ctx->d_ctc_sums);
        if (ctx->own_stream) hipStreamDestroy(ctx->stream);
        if (cn::t_opt == &ctx->opt) cn::t_opt = nullptr;
        delete ctx;
    });
}

int cn_ctx_set_option(cn_ctx *ctx, const char *name, int value)
{
    if (!ctx || !name) { g_last_error = "cn_ctx_set_option: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!strcmp(name, "deterministic")) { ctx->det = value != 0; return; }
        if (!strcmp(name, "overlap")) { ctx->overlap = value != 0; return; }
        if (option_set(ctx->opt, name, value)) return;
        throw cn_error(CN_ERR_BAD_ARG, std::string("cn_ctx_set_option: unknown option \"") + name + "\"");
    });
}

int cn_ctx_get_option(const cn_ctx *ctx, const char *name, int *value)
{
    if (!ctx || !name || !value) { g_last_error = "cn_ctx_get_option: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!strcmp(name, "deterministic")) { *value = ctx->det ? 1 : 0; return; }
        if (!strcmp(name, "overlap")) { *value = ctx->overlap ? 1 : 0; return; }
        long v = 0;
        if (option_get(ctx->opt, name, &v)) { *value = (int)v; return; }
        throw cn_error(CN_ERR_BAD_ARG, std::string("cn_ctx_get_option: unknown option \"") + name + "\"");
    });
}

int cn_ctx_synchronize(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_synchronize: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        join_side(ctx);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        HIP_CHECK(hipGetLastError());
        check_fault(ctx);
    });
}

int cn_ctx_join(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_join: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { enter(ctx); join_side(ctx); });
}

int cn_layer_join(cn_layer *layer)
{
    if (!layer) { g_last_error = "cn_layer_join: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        for (size_t i = 0; i < c->pending_joins.size(); ++i)
            if (c->pending_joins[i] == layer->ev_join) {
                HIP_CHECK(hipStreamWaitEvent(c->stream, layer->ev_join, 0));
                c->pending_joins.erase(c->pending_joins.begin() + i); c->pending_join_streams.erase(c->pending_join_streams.begin() + i);
                break;
            }
    });
}

void *cn_ctx_stream(cn_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int cn_layer_join_stream(cn_layer *layer, void *stream)
{
    if (!layer || !stream) { g_last_error = "cn_layer_join_stream: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(layer->ctx);
        stream_wait_layer(layer, (hipStream_t)stream);
    });
}

// ---------------------------------------------------------------------------------------------
// data-parallel training (RCCL)
// ---------------------------------------------------------------------------------------------
int cn_comm_unique_id(char *id)
{
    if (!id) { g_last_error = "cn_comm_unique_id: id is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        static_assert(sizeof(ncclUniqueId) == CN_COMM_ID_BYTES, "CN_COMM_ID_BYTES must match ncclUniqueId");
        if (ipc_backend_selected()) { ipc_unique_id(id, CN_COMM_ID_BYTES); return; }
        ncclUniqueId u;
        RCCL_CHECK(rccl().GetUniqueId(&u));
        memcpy(id, &u, sizeof(u));
    });
}

int cn_comm_init(cn_ctx *ctx, const char *id, int rank, int world)
{
    if (!ctx || !id) { g_last_error = "cn_comm_init: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (world < 1 || rank < 0 || rank >= world) throw cn_error(CN_ERR_BAD_ARG, "cn_comm_init: rank " + std::to_string(rank) + " outside world of " + std::to_string(world));
        if (ctx->has_comm()) throw cn_error(CN_ERR_STATE, "cn_comm_init: this context already has a communicator");
        enter(ctx);
        if (!ctx->comm_stream) {
            HIP_CHECK(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_comm, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_comm_fork, hipEventDisableTiming));
        }
        if (ipc_backend_selected()) {
            char fallback[CN_COMM_ID_BYTES];
            bool p2p_ok = true;
            try {
                ctx->ipc = ipc_comm_create(id, rank, world);
                // p2p: first contact.  Regions mapped, both forms of the exchange on a known bucket, one shared verdict.
                if (ipc_comm_is_p2p(ctx->ipc))
                    p2p_ok = ipc_comm_p2p_selfcheck(ctx->ipc, ctx->comm_stream, [](char *out) {
                        ncclUniqueId u;
                        rccl_check(rccl().GetUniqueId(&u), "ncclGetUniqueId");
                        memcpy(out, &u, sizeof(u));
                    }, fallback);
            }
            catch (const cn_error &) { if (ctx->ipc) { ipc_comm_mark_failed(ctx->ipc); ipc_comm_destroy(ctx->ipc); ctx->ipc = nullptr; } throw; }
            catch (const std::exception &e) {
                if (ctx->ipc) { ipc_comm_mark_failed(ctx->ipc); ipc_comm_destroy(ctx->ipc); ctx->ipc = nullptr; }
                throw cn_error(CN_ERR_COMM, e.what());
            }
            if (!p2p_ok) {
                // some rank saw a wrong sum or a time-out through a peer mapping: nobody trains on this backend.  Every rank got the
                // same verdict and the id rank 0 made: the job goes on over RCCL and says so.
                ipc_comm_destroy(ctx->ipc); ctx->ipc = nullptr;
                fprintf(stderr, "cn_comm_init: rank %d of %d: CN_COMM_BACKEND=p2p failed its first-contact self-check; falling back to RCCL\n", rank, world);
                ncclUniqueId u;
                memcpy(&u, fallback, sizeof(u));
                RCCL_CHECK(rccl().CommInitRank(&ctx->comm, world, u, rank));
            }
        } else {
            ncclUniqueId u;
            memcpy(&u, id, sizeof(u));
            RCCL_CHECK(rccl().CommInitRank(&ctx->comm, world, u, rank));
        }
        ctx->comm_rank = rank; ctx->comm_world = world;
    });
}

int cn_comm_destroy(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_comm_destroy: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!ctx->has_comm()) return;
        enter(ctx);
        HIP_CHECK(hipStreamSynchronize(ctx->comm_stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        std::string failure;
        if (ctx->ipc) {
            // p2p: a poll that timed out on the device is reported here at the latest (the resources go either way)
            try { ipc_comm_check(ctx->ipc, ctx->comm_stream); }
            catch (const std::exception &e) { ipc_comm_mark_failed(ctx->ipc); failure = e.what(); }
            ipc_comm_destroy(ctx->ipc); ctx->ipc = nullptr;
        }
        else RCCL_CHECK(rccl().CommDestroy(ctx->comm));
        ctx->comm = nullptr; ctx->comm_world = 0; ctx->comm_rank = 0; ctx->comm_pending = false;
        if (!failure.empty()) throw cn_error(CN_ERR_COMM, failure);
    });
}

int cn_comm_info(const cn_ctx *ctx, int *rank, int *world)
{
    if (!ctx) { g_last_error = "cn_comm_info: ctx is NULL"; return CN_ERR_BAD_ARG; }
    if (rank) *rank = ctx->comm_rank;
    if (world) *world = ctx->comm_world;
    return CN_OK;
}

const char *cn_comm_backend(const cn_ctx *ctx, int64_t *exchanges)
{
    if (exchanges) *exchanges = ctx ? ctx->comm_exchanges : 0;
    if (!ctx || !ctx->has_comm()) return "";
    return ctx->comm ? "rccl" : ipc_comm_is_p2p(ctx->ipc) ? "p2p" : "ipc";
}

// p2p: a wait inside an exchange kernel timed out (host-mapped word, no synchronisation): no update on top of a NaN gradient
static void comm_check_fast(cn_ctx *ctx)
{
    if (!ctx->ipc) return;
    try { ipc_comm_check_fast(ctx->ipc); }
    catch (const std::exception &e) { throw cn_error(CN_ERR_COMM, e.what()); }
}

// the ipc / p2p backends' exchange (ipc: host-blocking); a failure marks the segment so that the peers leave their barriers at once
static void ipc_reduce(cn_ctx *ctx, float *buf, size_t n)
{
    try { ipc_allreduce(ctx->ipc, buf, n, ctx->comm_stream, ctx->total); }
    catch (const std::exception &e) { ipc_comm_mark_failed(ctx->ipc); throw cn_error(CN_ERR_COMM, e.what()); }
}

int cn_allreduce_grads(cn_ctx *ctx, cn_layer *const *layers, int n)
{
    if (!ctx || n < 0 || (n > 0 && !layers)) { g_last_error = "cn_allreduce_grads: bad argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        refuse_swapped(ctx, "cn_allreduce_grads");
        require_comm(ctx, "cn_allreduce_grads");
        enter(ctx);
        finalize(ctx);
        ctx->clip_valid = false;
        // CN_COMM_TEST_DOUBLE (tests/test_gpu_parallel.py): the collective is replaced by a kernel on the communication stream
        // that doubles the gradient -- what a two-rank all-reduce of equal shards does --, so that the ORDER of gradient work,
        // exchange and update can be checked on a one-GPU box: a reduction that starts early or an update that does not wait
        // shows in the trained weights
        const bool test_double = opt().comm_test_double;
        if (test_double && ctx->comm_world > 1)
            throw cn_error(CN_ERR_STATE, "cn_allreduce_grads: CN_COMM_TEST_DOUBLE is set in a job of more than one rank (it replaces the "
                                         "gradient exchange by a stand-in and is for one-rank ordering tests only)");
        if (n == 0) {
            // the whole arena in one exchange: every gradient GEMM first, then fork the communication stream
            join_side(ctx);
            HIP_CHECK(hipEventRecord(ctx->ev_comm_fork, ctx->stream));
            HIP_CHECK(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_comm_fork, 0));
            float *g = ctx->arena + ctx->total;
            Timed tm(ctx, KC_COMM, ctx->comm_stream);
            ++ctx->comm_exchanges;
            if (test_double) launch_scale(ctx->comm_stream, g, ctx->total, 2.0f);
            else if (ctx->ipc) ipc_reduce(ctx, g, ctx->total);
            else if (ctx->total) RCCL_CHECK(rccl().AllReduce(g, g, ctx->total, ncclFloat32, ncclSum, ctx->comm, ctx->comm_stream));
        } else {
            for (int i = 0; i < n; ++i) {
                cn_layer *l = layers[i];
                if (!l || l->ctx != ctx || !l->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_allreduce_grads: not a trainable layer of this context");
                stream_wait_layer(l, ctx->comm_stream);
                Timed tm(ctx, KC_COMM, ctx->comm_stream);          // (events on the communication stream: the exchange itself, not its wait)
                ++ctx->comm_exchanges;
                if (test_double) launch_scale(ctx->comm_stream, l->wu, (size_t)l->nw, 2.0f);
                else if (ctx->ipc) ipc_reduce(ctx, l->wu, (size_t)l->nw);
                else RCCL_CHECK(rccl().AllReduce(l->wu, l->wu, (size_t)l->nw, ncclFloat32, ncclSum, ctx->comm, ctx->comm_stream));
                // armed update: the layer's step follows its reduction on the communication stream
                if (ctx->armed && !l->updated) launch_layer_update(ctx->comm_stream, l, 1, ctx->arm, nullptr);
            }
        }
        HIP_CHECK(hipEventRecord(ctx->ev_comm, ctx->comm_stream));
        ctx->comm_pending = true;
    });
}

// ---------------------------------------------------------------------------------------------
// layers
// ---------------------------------------------------------------------------------------------
int cn_layer_create(cn_ctx *ctx, cn_layer_kind kind, cn_layer *preceding, int size, float bias,
                    int parallel_sequences, int max_seq_length, cn_layer **out)
{
    if (!ctx || !out) { g_last_error = "cn_layer_create: NULL argument"; return CN_ERR_BAD_ARG; }
    *out = nullptr;
    cn_layer *l = nullptr;
    int rc = guarded([&] {
        enter(ctx);
        if (size <= 0) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: layer size must be positive");
        if (kind == CN_LAYER_CONTEXT) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: a context layer has members of its own: use cn_layer_create_context");
        if (kind == CN_LAYER_INPUT) {
            if (preceding) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: the input layer has no preceding layer");
            if (parallel_sequences <= 0 || max_seq_length <= 0)
                throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: parallel_sequences and max_seq_length must be positive");
            if (ctx->PS) throw cn_error(CN_ERR_STATE, "cn_layer_create: this context already has an input layer");
        } else {
            if (!preceding) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: preceding layer required");
            if (preceding->ctx != ctx) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: preceding layer belongs to another context");
            if (preceding->post) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: a post output layer must be the last layer");
        }
        l = new cn_layer;
        l->ctx = ctx; l->kind = kind; l->prev = preceding; l->size = size; l->bias = bias;
        l->ordinal = ctx->next_ordinal;
        l->PS = preceding ? preceding->PS : parallel_sequences;
        l->maxT = preceding ? preceding->maxT : max_seq_length;
        l->ax = preceding ? preceding->ax : &ctx->base;
        if (!preceding) {
            // sequences per workgroup of the recurrent kernels: the fewest (4, 8, 16) that still give at most
            // one workgroup per CU for a bidirectional layer; PS is padded to a whole number of groups
            const int cus = ctx->num_cus;
            int rpl = ctx->rpl_override ? ctx->rpl_override : (2 * ((l->PS + 3) / 4) <= cus ? 1 : (2 * ((l->PS + 7) / 8) <= cus ? 2 : 4));
            if (rpl != 1 && rpl != 2 && rpl != 4) throw cn_error(CN_ERR_BAD_ARG, "CN_RPL must be 1, 2 or 4");
            ctx->rpl = rpl;
            ctx->PSp = round_up(l->PS, 4 * rpl);
        }
        l->PSp = ctx->PSp;
        const size_t maxN = l->maxN(), e = ctx->esz();
        if (preceding) { l->P = preceding->size; l->Pp = preceding->Lp; }

        switch (kind) {
        case CN_LAYER_INPUT: {
            l->Lp = round_up(size, 32);
            l->stage_in = (float *)dalloc(l, maxN * size * sizeof(float));
            l->out_op = dalloc(l, maxN * l->Lp * e);
            ctx->PS = l->PS; ctx->maxT = l->maxT;
            {   // pattern types, with guard steps of PATTYPE_NONE on both sides (dalloc_guarded)
                const size_t guard = (size_t)CN_GUARD_STEPS * ctx->PSp;
                HIP_CHECK(hipMalloc((void **)&ctx->d_pat_raw, cn_ctx::pat_bytes(maxN, guard)));
                HIP_CHECK(hipMemsetAsync(ctx->d_pat_raw, 0, cn_ctx::pat_bytes(maxN, guard), ctx->stream));   // pad slots: PATTYPE_NONE forever
                ctx->pat_maxN = maxN; ctx->pat_guard = guard;
                ctx->d_pat = ctx->d_pat_raw + guard;
            }
            HIP_CHECK(hipMalloc((void **)&ctx->d_tcls, maxN * sizeof(int)));
            HIP_CHECK(hipMemsetAsync(ctx->d_tcls, 0xFF, maxN * sizeof(int), ctx->stream));     // pad slots: target class -1
            sync_base(ctx);
            break; }
        case CN_LAYER_LSTM:
        case CN_LAYER_BLSTM: {
            if (ctx->finalized) throw cn_error(CN_ERR_STATE, "cn_layer_create: parameter arena already laid out");
            l->lstm = true; l->trainable = true;
            l->dirs = (kind == CN_LAYER_BLSTM) ? 2 : 1;
            if (l->dirs == 2 && size % 2 != 0)
                throw cn_error(CN_ERR_SHAPE, "Cannot create a bidirectional layer with an odd layer size");   // LstmLayer.cu:528-529
            l->H = size / l->dirs; l->Hp = pad_units(l->H);
            // bf16 mode: widths between the register-resident shapes (<= 192) and a cluster shape (256, 512) are padded
            // up to the cluster shape when the cluster fits the chip: zero units cost GEMM work and memory, streaming
            // W_rec from L2 every time step costs an order of magnitude more
            if (!ctx->f32 && l->Hp > 192 && l->Hp < 512 && l->Hp != 256) {
                const int hc = l->Hp < 256 ? 256 : 512;
                if (lstm_cluster_xch_bytes(P_BF16, hc, l->dirs, ctx->PSp, ctx->rpl, ctx->num_cus) > 0) l->Hp = hc;
            }
            // split-bf16 mode: the same between the register-resident shapes (<= 128) and its one cluster shape (256)
            if (ctx->prec == P_X3 && l->Hp > 128 && l->Hp < 256 &&
                lstm_cluster_xch_bytes(P_X3, 256, l->dirs, ctx->PSp, ctx->rpl, ctx->num_cus) > 0) l->Hp = 256;
            l->Lp = l->dirs * l->Hp;
            const size_t R = (size_t)l->dirs * 4 * l->Hp;
            // the recurrent kernels address every per-frame buffer with 32-bit byte offsets from its base
            if (maxN * R * sizeof(float) >= (1ull << 32))
                throw cn_error(CN_ERR_SHAPE, "cn_layer_create: parallel_sequences * max_seq_length * 16 * layer size must stay below 4 GiB "
                                             "per LSTM layer; use fewer parallel sequences");
            l->nw = size * (4 * (l->P + 1) + 4 * l->H + 3);                                            // LstmLayer.cu:525
            l->out_op = dalloc(l, maxN * l->Lp * e);
            l->err = (float *)dalloc_guarded(l, maxN * l->Lp * sizeof(float), (size_t)ctx->PSp * l->Lp * sizeof(float));
            l->acts = (float *)dalloc_guarded(l, maxN * R * sizeof(float), (size_t)ctx->PSp * R * sizeof(float));
            if (ctx->prec == P_BF16) l->pre16 = dalloc_guarded(l, maxN * R * 2, (size_t)ctx->PSp * R * 2);
            l->cell = (float *)dalloc_guarded(l, maxN * l->Lp * sizeof(float), (size_t)ctx->PSp * l->Lp * sizeof(float));
            l->th = (float *)dalloc_guarded(l, maxN * l->Lp * sizeof(float), (size_t)ctx->PSp * l->Lp * sizeof(float));
            l->delta_op = dalloc(l, maxN * R * e);
            l->Win = dalloc(l, R * l->Pp * e); l->WinT = dalloc(l, R * l->Pp * e);
            l->Wrec = dalloc(l, R * l->Hp * e); l->WrecT = dalloc(l, R * l->Hp * e);
            l->bias_p = (float *)dalloc(l, R * sizeof(float));
            l->peep_p = (float *)dalloc(l, (size_t)l->dirs * 3 * l->Hp * sizeof(float));
            l->grad_block_floats = R * l->Pp + R * l->Hp + R + (size_t)l->dirs * 3 * l->Hp;
            l->grad_block = (float *)dalloc(l, l->grad_block_floats * sizeof(float));
            l->dWin = l->grad_block; l->dWrec = l->dWin + R * l->Pp; l->dbias = l->dWrec + R * l->Hp; l->dpeep = l->dbias + R;
            {   // exchange buffer of the multi-CU cluster kernels (layers whose W_rec exceeds one CU)
                const size_t xb = lstm_cluster_xch_bytes(ctx->prec, l->Hp, l->dirs, ctx->PSp, ctx->rpl, ctx->num_cus);
                if (xb > ctx->xch_bytes) {
                    if (ctx->d_xch) HIP_CHECK(hipFree(ctx->d_xch));
                    HIP_CHECK(hipMalloc((void **)&ctx->d_xch, xb));
                    HIP_CHECK(hipMemsetAsync(ctx->d_xch, 0, xb, ctx->stream));
                    ctx->xch_bytes = xb; ctx->xch_epoch = 0;
                }
            }
            break; }
        case CN_LAYER_FF_TANH:
        case CN_LAYER_FF_LOGISTIC:
        case CN_LAYER_FF_IDENTITY:
        case CN_LAYER_SOFTMAX: {
            if (ctx->finalized) throw cn_error(CN_ERR_STATE, "cn_layer_create: parameter arena already laid out");
            l->trainable = true;
            l->Lp = round_up(size, 32);
            l->nw = size * (l->P + 1);                                                                   // FeedForwardLayer.cu:130
            l->out_f32 = (float *)dalloc(l, maxN * l->Lp * sizeof(float));
            l->out_op = ctx->f32 ? (void *)l->out_f32 : dalloc(l, maxN * l->Lp * e);
            l->err = (float *)dalloc(l, maxN * l->Lp * sizeof(float));
            l->delta_op = ctx->f32 ? (void *)l->err : dalloc(l, maxN * l->Lp * e);
            l->Win = dalloc(l, (size_t)l->Lp * l->Pp * e); l->WinT = dalloc(l, (size_t)l->Lp * l->Pp * e);
            l->bias_p = (float *)dalloc(l, l->Lp * sizeof(float));
            l->grad_block_floats = (size_t)l->Lp * l->Pp + l->Lp;
            l->grad_block = (float *)dalloc(l, l->grad_block_floats * sizeof(float));
            l->dWin = l->grad_block; l->dbias = l->dWin + (size_t)l->Lp * l->Pp;
            if (kind == CN_LAYER_SOFTMAX && softmax_fwd_can_be_lazy(size)) l->sm_stat = (float *)dalloc(l, maxN * 2 * sizeof(float));
            break; }
        case CN_LAYER_SSE:
        case CN_LAYER_WEIGHTEDSSE:
        case CN_LAYER_SSE_MASK:
        case CN_LAYER_CE:
        case CN_LAYER_RMSE:
        case CN_LAYER_BINARY_CLASSIFICATION:
        case CN_LAYER_MULTICLASS_CLASSIFICATION: {
            if (!preceding->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: a post output layer needs a trainable preceding layer");
            if (preceding->lstm) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: post output layers directly after an LSTM layer are not supported");
            if (preceding->residual) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: a post output layer directly after a residual layer is not supported");
            const bool paired = kind == CN_LAYER_WEIGHTEDSSE || kind == CN_LAYER_SSE_MASK;
            // PostOutputLayer.cpp:58-59; the weighted layers take (target, weight) pairs: WeightedSsePostOutputLayer.cu:103, SseMaskPostOutputLayer.cu:103
            if (paired ? size != 2 * preceding->size : size != preceding->size)
                throw cn_error(CN_ERR_SHAPE, "Size mismatch: " + std::to_string(size) + " vs. " + std::to_string(preceding->size));
            if (kind == CN_LAYER_BINARY_CLASSIFICATION && size != 1)                                      // BinaryClassificationLayer.cu:123-124
                throw cn_error(CN_ERR_SHAPE, "The binary classification post output layer cannot be used for an output layer size != 1");
            if (kind == CN_LAYER_MULTICLASS_CLASSIFICATION && size == 1)                                  // MulticlassClassificationLayer.cu:146-147
                throw cn_error(CN_ERR_SHAPE, "The multiclass classification post output layer cannot be used for an output layer size of 1");
            l->post = true; l->Lp = preceding->Lp;
            // (every post output layer: the per-pattern terms of its error pass through here and are summed in a fixed order)
            if (kind == CN_LAYER_MULTICLASS_CLASSIFICATION && !ctx->d_rowstat)
                HIP_CHECK(hipMalloc((void **)&ctx->d_rowstat, maxN * 2 * sizeof(float)));
            if (kind != CN_LAYER_MULTICLASS_CLASSIFICATION) {
                // (the loads fill `targets` at the base rate; behind a strided layer the rows of the layer's axis are gathered from them)
                l->targets = (float *)dalloc(l, (size_t)ctx->PSp * ctx->maxT * size * sizeof(float));
                if (l->ax->owner) l->ax_targets = (float *)dalloc(l, maxN * size * sizeof(float));
                if (!ctx->d_rowstat) HIP_CHECK(hipMalloc((void **)&ctx->d_rowstat, maxN * 2 * sizeof(float)));
            }
            break; }
        case CN_LAYER_CTC: {
            if (preceding->kind != CN_LAYER_SOFTMAX) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: a ctc layer needs a softmax layer as its preceding layer");
            if (size != preceding->size) throw cn_error(CN_ERR_SHAPE, "Size mismatch: " + std::to_string(size) + " vs. " + std::to_string(preceding->size));
            if (size < 2) throw cn_error(CN_ERR_SHAPE, "The ctc post output layer needs at least one label and the blank (output layer size >= 2)");
            l->post = true; l->Lp = preceding->Lp;
            const long cap = opt().ctc_max_labels > 0 ? opt().ctc_max_labels : std::min(l->maxT, 512);
            if (!ctc_shape_fits((int)std::min<long>(cap, CTC_MAX_STATES), l->Lp) || cap > CTC_MAX_STATES)
                throw cn_error(CN_ERR_SHAPE, "cn_layer_create: a ctc layer with " + std::to_string(cap) + " labels per sequence (option ctc_max_labels) and " +
                                             std::to_string(size) + " units does not fit a workgroup (2 * labels + 1 <= " + std::to_string(CTC_MAX_STATES) +
                                             " states, 2 * (2 * labels + 1) + padded units <= 15360 floats of LDS)");
            l->ctc_cap = (int)cap;
            const size_t nlab = (size_t)l->ctc_cap * l->PS;
            l->ctc_labels = (int *)dalloc(l, (3 * nlab + l->PSp + 1) * sizeof(int));
            l->ctc_Sp = round_up(2 * l->ctc_cap + 1, 64);
            l->ctc_alpha = (int2 *)dalloc(l, (size_t)l->PSp * l->maxT * l->ctc_Sp * sizeof(int2));
            l->ctc_beta = (int2 *)dalloc(l, (size_t)l->PSp * l->maxT * l->ctc_Sp * sizeof(int2));
            l->ctc_info = (int *)dalloc(l, (size_t)l->PSp * 2 * sizeof(int));
            l->ctc_rowstat = (float *)dalloc(l, (size_t)l->PSp * 2 * sizeof(float));
            break; }
        default:
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create: unknown layer kind");
        }
        if (preceding && l->trainable) preceding->has_follower = true;
        ctx->layers.push_back(l);
        ++ctx->next_ordinal;
    });
    if (rc != CN_OK) { if (l) { for (void *p : l->owned) hipFree(p); delete l; } return rc; }
    *out = l;
    return CN_OK;
}

int cn_layer_create_context(cn_ctx *ctx, cn_layer *preceding, int left, int right, int dilation, cn_layer **out)
{
    return cn_layer_create_context_strided(ctx, preceding, left, right, dilation, 1, out);
}

int cn_layer_create_context_strided(cn_ctx *ctx, cn_layer *preceding, int left, int right, int dilation, int stride, cn_layer **out)
{
    if (!ctx || !out) { g_last_error = "cn_layer_create_context: NULL argument"; return CN_ERR_BAD_ARG; }
    *out = nullptr;
    cn_layer *l = nullptr;
    int rc = guarded([&] {
        enter(ctx);
        if (!preceding) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context: preceding layer required");
        if (preceding->ctx != ctx) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context: preceding layer belongs to another context");
        if (preceding->post) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context: a post output layer must be the last layer");
        if (left < 0 || left > 32 || right < 0 || right > 32)
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context: left and right must lie in 0..32 (" + std::to_string(left) + ", " + std::to_string(right) + ")");
        if (dilation < 1 || dilation > 16)
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context: dilation must lie in 1..16 (" + std::to_string(dilation) + ")");
        if (stride < 1 || stride > 8)
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_create_context_strided: stride must lie in 1..8 (" + std::to_string(stride) + ")");
        l = new cn_layer;
        l->ctx = ctx; l->kind = CN_LAYER_CONTEXT; l->prev = preceding; l->context = true;
        l->cx_left = left; l->cx_right = right; l->cx_dil = dilation;
        l->ordinal = ctx->next_ordinal;
        l->cx_stride = stride;
        l->PS = preceding->PS; l->maxT = ceil_div(preceding->maxT, stride); l->PSp = ctx->PSp;
        l->ax = preceding->ax;
        l->P = preceding->size; l->Pp = preceding->Lp;
        l->size = (left + right + 1) * l->P;
        l->Lp = round_up(l->size, 32);                    // dense rows, whatever padding the preceding layer's have
        const size_t maxN = l->maxN();
        l->out_op = dalloc(l, maxN * l->Lp * ctx->esz());
        l->err = (float *)dalloc(l, maxN * l->Lp * sizeof(float));
        if (!ctx->cx_len) {
            HIP_CHECK(hipMalloc((void **)&ctx->cx_len, (size_t)l->PSp * sizeof(int)));
            HIP_CHECK(hipMemsetAsync(ctx->cx_len, 0, (size_t)l->PSp * sizeof(int), ctx->stream));
        }
        if (stride > 1) {
            // the layer's own axis: pattern types between CN_GUARD_STEPS of NONE on both sides with the row map behind them, as the
            // context's (cn_layer_create's input case; the recurrent loops of a follower prefetch outside [0, T')), classes, lengths
            TimeAxis &ax = l->own_axis;
            const size_t guard = (size_t)CN_GUARD_STEPS * ctx->PSp;
            ax.maxT = l->maxT; ax.rate = preceding->ax->rate * stride; ax.owner = l;
            ax.pat_maxN = maxN; ax.pat_guard = guard;
            ax.pat_raw = (char *)dalloc(l, cn_ctx::pat_bytes(maxN, guard));
            ax.pat = ax.pat_raw + guard;
            ax.tcls = (int *)dalloc(l, maxN * sizeof(int));
            HIP_CHECK(hipMemsetAsync(ax.tcls, 0xFF, maxN * sizeof(int), ctx->stream));
            ax.len = (int *)dalloc(l, (size_t)l->PSp * sizeof(int));
            l->ax = &ax;
        }
        sync_base(ctx);                                   // (the base axis names cx_len)
        preceding->has_follower = true;                   // (a feed-forward or softmax predecessor keeps its operand copy for the gather)
        ctx->layers.push_back(l);
        ++ctx->next_ordinal;
    });
    if (rc != CN_OK) { if (l) { for (void *p : l->owned) hipFree(p); delete l; } return rc; }
    *out = l;
    return CN_OK;
}

int cn_layer_context(const cn_layer *layer, int *left, int *right, int *dilation)
{
    if (!layer || !layer->context) { g_last_error = "cn_layer_context: not a context layer"; return CN_ERR_BAD_ARG; }
    if (left) *left = layer->cx_left;
    if (right) *right = layer->cx_right;
    if (dilation) *dilation = layer->cx_dil;
    return CN_OK;
}

int cn_layer_context_stride(const cn_layer *layer, int *stride)
{
    if (!layer || !layer->context) { g_last_error = "cn_layer_context_stride: not a context layer"; return CN_ERR_BAD_ARG; }
    if (stride) *stride = layer->cx_stride;
    return CN_OK;
}

int cn_layer_time(const cn_layer *layer, int *T, int *Tmin, int *rate)
{
    if (!layer) { g_last_error = "cn_layer_time: layer is NULL"; return CN_ERR_BAD_ARG; }
    if (!layer->ctx->loaded) { g_last_error = "cn_layer_time: no fraction loaded (call cn_fraction_load first)"; return CN_ERR_STATE; }
    // host arithmetic from the base axis: what the strided layers in front form, whether they have run or not
    const int r = layer->ax->rate;
    if (T) *T = ceil_div(layer->ctx->T, r);
    if (Tmin) *Tmin = ceil_div(layer->ctx->Tmin, r);
    if (rate) *rate = r;
    return CN_OK;
}

int cn_layer_destroy(cn_layer *layer)
{
    if (!layer) return CN_OK;
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        join_side(c);                                   // side-stream work of this layer may still be in flight
        HIP_CHECK(hipStreamSynchronize(c->stream));
        if (c->side) HIP_CHECK(hipStreamSynchronize(c->side));      // (operand copies being rebuilt: ev_pack_last may be this layer's)
        for (cn_layer *o : c->layers) o->pack_pending = false;
        c->ev_pack_last = nullptr;
        for (void *p : layer->owned) hipFree(p);
        if (layer->ev_fork) { hipEventDestroy(layer->ev_fork); hipEventDestroy(layer->ev_join); }
        if (layer->ev_pack) hipEventDestroy(layer->ev_pack);
        for (int b = 0; b < 2; ++b) if (layer->ctc_hbuf[b]) { hipHostFree(layer->ctc_hbuf[b]); hipEventDestroy(layer->ctc_ev[b]); }
        if (c->rowstat_of == layer) c->rowstat_of = nullptr;
        for (size_t i = 0; i < c->layers.size(); ++i)
            if (c->layers[i] == layer) { c->layers.erase(c->layers.begin() + i); break; }
        delete layer;
    });
}

int cn_layer_size(const cn_layer *layer) { return layer ? layer->size : CN_ERR_BAD_ARG; }
int cn_layer_kind_of(const cn_layer *layer) { return layer ? (int)layer->kind : CN_ERR_BAD_ARG; }
int cn_layer_weight_count(const cn_layer *layer) { return layer ? layer->nw : CN_ERR_BAD_ARG; }

// ---------------------------------------------------------------------------------------------
// fraction
// ---------------------------------------------------------------------------------------------
static void check_fraction(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    if (input->kind != CN_LAYER_INPUT) throw cn_error(CN_ERR_BAD_ARG, "cn_fraction_load: `input` is not an input layer");
    const cn_input_splice &sp = ctx->splice;
    if (splice_enabled(sp)) {      // a source-rate fraction of unspliced patterns (section Input splicing and frame skipping)
        const int B = sp.context_left + sp.context_right + 1;
        if (input->size % B != 0)
            throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: input layer size of " + std::to_string(input->size) + " is no multiple of the " +
                           std::to_string(B) + " frames of the input splicing's context");
        if (f->input_pattern_size != input->size / B)
            throw cn_error(CN_ERR_SHAPE, "Input layer size of " + std::to_string(input->size) + " / " + std::to_string(B) + " spliced frames = " +
                           std::to_string(input->size / B) + " != data input pattern size of " + std::to_string(f->input_pattern_size));
    } else if (f->input_pattern_size != input->size)                                              // InputLayer.cpp:52-55
        throw cn_error(CN_ERR_SHAPE, "Input layer size of " + std::to_string(input->size) +
                       " != data input pattern size of " + std::to_string(f->input_pattern_size));
    if (post_output) {
        if (!post_output->post) throw cn_error(CN_ERR_BAD_ARG, "cn_fraction_load: `post_output` is not a post output layer");
        if (post_output->kind != CN_LAYER_CTC && f->output_pattern_size != post_output->size)                                          // PostOutputLayer.cpp:70-73
            throw cn_error(CN_ERR_SHAPE, "Output layer size of " + std::to_string(post_output->size) +
                           " != data target pattern size of " + std::to_string(f->output_pattern_size));
    }
    const int T = f->max_seq_length;
    if (T > 0 && splice_enabled(sp) && ceil_div(T, sp.frame_skip) > ctx->maxT)
        throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: max_seq_length " + std::to_string(T) + " at a frame skip of " + std::to_string(sp.frame_skip) +
                       " gives " + std::to_string(ceil_div(T, sp.frame_skip)) + " steps, outside (0, " + std::to_string(ctx->maxT) + "]");
    if (T <= 0 || (!splice_enabled(sp) && T > ctx->maxT)) throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: max_seq_length " + std::to_string(T) +
                                                " outside (0, " + std::to_string(ctx->maxT) + "]");
    if (f->min_seq_length < 0 || f->min_seq_length > T) throw cn_error(CN_ERR_SHAPE, "cn_fraction_load: bad min_seq_length");
    if (!f->pat_types || !f->inputs) throw cn_error(CN_ERR_BAD_ARG, "cn_fraction_load: pat_types / inputs missing");
}
static void require_targets(const char *fn, const cn_layer *post, const cn_fraction *f)
{
    if (!post) return;
    const bool cls = is_class_post(post);
    if (cls ? !f->target_classes : !f->targets) throw cn_error(CN_ERR_BAD_ARG, std::string(fn) + (cls ? ": target_classes missing" : ": targets missing"));
}
// Host buffers of a fraction -> pinned staging area -> ONE contiguous upload on the copy stream ([patTypes | classes or targets |
// inputs]; the two staging areas alternate).  Returns the area and the fraction with its pointers into it; ev_up[slot] completes
// with the upload.
struct Staged { int slot; cn_fraction f; };
static Staged stage_upload(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    const int T = f->max_seq_length;
    const size_t PS = ctx->PS;
    const bool cls = is_class_post(post_output);
    const size_t rows = (size_t)T * PS;
    const size_t W = post_output ? (size_t)post_output->size : 0;
    const size_t b_pat = (rows + 15) & ~(size_t)15;
    const size_t b_tgt = !post_output ? 0 : (cls ? rows * sizeof(int) : rows * W * sizeof(float));
    const size_t b_tgt_al = (b_tgt + 15) & ~(size_t)15;
    const size_t b_in = rows * (size_t)f->input_pattern_size * sizeof(float);      // (the input layer's size, or P0 of a spliced load: check_fraction)
    const size_t need = b_pat + b_tgt_al + b_in;
    if (need > ctx->stage_bytes || !ctx->h_stage[0]) {
        HIP_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < 2; ++i) {
            if (ctx->h_stage[i]) HIP_CHECK(hipHostFree(ctx->h_stage[i]));
            if (ctx->d_stage[i]) HIP_CHECK(hipFree(ctx->d_stage[i]));
            ctx->stage_used[i] = false;
        }
        // (the longest fraction the layers take: maxT steps, at source rate frame_skip times as many of the narrower patterns --
        // under the splice setting in force now: a later setting that needs more comes back here, at the price of this synchronise)
        const size_t maxrows = (size_t)ctx->maxT * PS * (splice_enabled(ctx->splice) ? (size_t)ctx->splice.frame_skip : 1);
        size_t cap = ((maxrows + 15) & ~(size_t)15) + ((maxrows * std::max(W * sizeof(float), sizeof(int)) + 15) & ~(size_t)15) + maxrows * (size_t)f->input_pattern_size * sizeof(float);
        if (cap < need) cap = need;
        for (int i = 0; i < 2; ++i) {
            HIP_CHECK(hipHostMalloc((void **)&ctx->h_stage[i], cap, hipHostMallocDefault));
            HIP_CHECK(hipMalloc((void **)&ctx->d_stage[i], cap));
            if (!ctx->ev_up[i]) { HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_up[i], hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_free[i], hipEventDisableTiming)); }
        }
        if (!ctx->copy) HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
        ctx->stage_bytes = cap;
    }
    const int slot = (int)(ctx->upload_idx++ & 1u);
    if (ctx->stage_used[slot]) HIP_CHECK(hipEventSynchronize(ctx->ev_free[slot]));    // the re-layout kernel two fractions ago has read it
    char *h = ctx->h_stage[slot], *dv = ctx->d_stage[slot];
    memcpy(h, f->pat_types, rows);
    if (post_output) memcpy(h + b_pat, cls ? (const void *)f->target_classes : (const void *)f->targets, b_tgt);
    memcpy(h + b_pat + b_tgt_al, f->inputs, b_in);
    HIP_CHECK(hipMemcpyAsync(dv, h, need, hipMemcpyHostToDevice, ctx->copy));
    HIP_CHECK(hipEventRecord(ctx->ev_up[slot], ctx->copy));
    Staged sg{slot, *f};
    sg.f.pat_types = dv;
    sg.f.target_classes = (post_output && cls) ? (const int *)(dv + b_pat) : nullptr;
    sg.f.targets = (post_output && !cls) ? (const float *)(dv + b_pat) : nullptr;
    sg.f.inputs = (const float *)(dv + b_pat + b_tgt_al);
    return sg;
}

static bool same_fraction(const cn_fraction &a, const cn_fraction &b)
{
    return a.max_seq_length == b.max_seq_length && a.min_seq_length == b.min_seq_length && a.num_sequences == b.num_sequences &&
           a.input_pattern_size == b.input_pattern_size && a.output_pattern_size == b.output_pattern_size &&
           a.pat_types == b.pat_types && a.inputs == b.inputs && a.target_classes == b.target_classes && a.targets == b.targets;
}
// `f` is the current fraction from here on
static void set_current(cn_ctx *ctx, const cn_fraction *f)
{
    const int T = f->max_seq_length;
    ctx->T = T; ctx->Tmin = f->min_seq_length; ctx->N = T * ctx->PSp; ctx->Next = T * ctx->PS; ctx->numSeqs = f->num_sequences;
    ctx->est_real = f->num_sequences * ((f->min_seq_length + T + 1) / 2);
    ctx->loaded = true;
    ++ctx->frac_serial;
    sync_base(ctx);
}
// the alternate buffers a prefetch re-laid its fraction out into become the current ones
static void swap_in_prefetched(cn_ctx *ctx, cn_layer *input, cn_layer *post_output)
{
    cn_ctx::Prefetch &pf = ctx->pf;
    std::swap(ctx->d_pat, pf.pat); std::swap(ctx->d_pat_raw, pf.pat_raw); std::swap(ctx->d_tcls, pf.tcls);
    std::swap(input->out_op, pf.in_op);
    if (post_output && post_output->targets) std::swap(post_output->targets, pf.targets);
}
// a CTC layer takes no targets from the fraction (cn_layer_set_label_sequences brings its labels): the data paths below see none
static cn_layer *target_taker(cn_layer *post_output)
{
    return post_output && post_output->kind == CN_LAYER_CTC ? nullptr : post_output;
}
static int fraction_load(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f, bool resident)
{
    if (!ctx || !input || !f) { g_last_error = "cn_fraction_load: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        check_fraction(ctx, input, post_output, f);
        post_output = target_taker(post_output);
        const int T = f->max_seq_length;
        finalize(ctx);
        join_side(ctx);                      // gradient GEMMs of the previous fraction still read the activations
        flush_loss(ctx);                     // (a deferred loss sum counts the rows of the fraction that is being replaced)
        Timed tm(ctx, KC_OTHER);
        require_targets("cn_fraction_load", post_output, f);
        check_augment_shape(ctx->aug, ctx->splice, input);
        const bool spliced = splice_enabled(ctx->splice);
        cn_ctx::Prefetch &pf = ctx->pf;
        // a prefetch of the same kind (resident / host buffers) announced exactly this fraction and the side stream has re-laid it
        // out (join_side above ordered this stream behind it): nothing is copied or launched here
        const bool hit = pf.valid && pf.launched && pf.host == !resident && pf.input == input && pf.post == post_output &&
                         same_fraction(pf.host ? pf.f_host : pf.f, *f) && same_augment(pf.aug, ctx->aug) &&
                         same_splice(pf.splice, ctx->splice);
        pf.valid = false;          // a prefetch serves the very next load or nothing
        const FractionBuffers cur{ctx->d_pat, ctx->d_pat_raw, ctx->d_tcls, input->out_op, post_output ? post_output->targets : nullptr};
        if (hit) {
            ++pf.hits;
            swap_in_prefetched(ctx, input, post_output);
        } else if (resident) {      // everything is in HBM already: one kernel re-lays it out
            relayout(ctx->stream, ctx, input, post_output, *f, cur, ctx->aug, ctx->splice, ctx->aug_tab);
        } else if (ctx->overlap || spliced) {
            // Host buffers: pack [patTypes | classes or targets | inputs] into pinned memory, ONE contiguous upload
            // on the copy stream (it runs while the previous fraction still computes: the staging areas alternate),
            // then the same re-layout kernel as the resident path.  (Strided 2-D copies from pageable memory cost
            // one transfer per time step: 3.5 ms per fraction of 2.3 MB, twice the whole training step.)
            const Staged sg = stage_upload(ctx, input, post_output, f);
            relayout_staged(ctx->stream, ctx, input, post_output, sg.f, cur, sg.slot, ctx->aug, ctx->splice, ctx->aug_tab);
            // (option overlap = 0 with splicing on: the same route and the same kernel, then the wait its strided copies end with)
            if (!ctx->overlap) HIP_CHECK(hipStreamSynchronize(ctx->stream));
        } else {
            // CN_NO_OVERLAP: strided copies [T][PS] -> [T][PSp]: pad slots keep their permanent NONE / -1 / 0 contents
            const size_t PS = ctx->PS, PSp = ctx->PSp;
            const int N = T * (int)PSp;
            const hipMemcpyKind kind = hipMemcpyHostToDevice;
            HIP_CHECK(hipMemcpy2DAsync(ctx->d_pat, PSp, f->pat_types, PS, PS, T, kind, ctx->stream));
            launch_rowmap(ctx->stream, ctx->d_pat, N, ctx->rowmap_of(ctx->d_pat_raw), (int)ctx->pat_maxN, f->min_seq_length * (int)PSp);
            const size_t irow = (size_t)input->size * sizeof(float);
            HIP_CHECK(hipMemcpy2DAsync(input->stage_in, PSp * irow, f->inputs, PS * irow, PS * irow, T, kind, ctx->stream));
            if (is_class_post(post_output)) {
                HIP_CHECK(hipMemcpy2DAsync(ctx->d_tcls, PSp * sizeof(int), f->target_classes, PS * sizeof(int), PS * sizeof(int), T, kind, ctx->stream));
                if (post_output->kind == CN_LAYER_BINARY_CLASSIFICATION)
                    launch_classes_to_targets(ctx->stream, ctx->d_tcls, post_output->targets, N);
            } else if (post_output) {
                const size_t trow = (size_t)post_output->size * sizeof(float);
                HIP_CHECK(hipMemcpy2DAsync(post_output->targets, PSp * trow, f->targets, PS * trow, PS * trow, T, kind, ctx->stream));
            }
            if (aug_enabled(ctx->aug)) {       // the same arithmetic at the pad_convert stage, from the pattern types just copied
                ensure_aug_table(ctx, ctx->aug_tab);
                const AugArgs g = aug_args(ctx->aug, input);
                launch_augment_table(ctx->stream, g, ctx->d_pat, (int)PSp, T, (int)PS, ctx->aug_tab);
                launch_pad_convert_augment(ctx->stream, ctx->f32, g, ctx->aug_tab, input->stage_in, ctx->d_pat, T, (int)PS, (int)PSp,
                                           input->size, input->out_op, input->Lp);
            } else {
                launch_pad_convert(ctx->stream, ctx->f32, input->stage_in, N, input->size, input->out_op, input->Lp);
            }
            HIP_CHECK(hipStreamSynchronize(ctx->stream));     // the caller may reuse its host buffers on return
        }
        const cn_fraction fnet = network_rate(ctx->splice, *f);
        set_current(ctx, &fnet);
        for (cn_layer *l : ctx->layers) l->ctc_labels_valid = l->ctc_swept = false;      // the labels belonged to the fraction that has been replaced
    });
}

int cn_fraction_load(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    return fraction_load(ctx, input, post_output, f, false);
}
int cn_fraction_load_resident(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    return fraction_load(ctx, input, post_output, f, true);
}
static int fraction_prefetch(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f, bool host);
int cn_fraction_prefetch_resident(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    return fraction_prefetch(ctx, input, post_output, f, false);
}
int cn_fraction_prefetch(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f)
{
    return fraction_prefetch(ctx, input, post_output, f, true);
}
static int fraction_prefetch(cn_ctx *ctx, cn_layer *input, cn_layer *post_output, const cn_fraction *f, bool host)
{
    if (!ctx || !input || !f) { g_last_error = "cn_fraction_prefetch_resident: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        check_fraction(ctx, input, post_output, f);
        post_output = target_taker(post_output);
        if (host && !ctx->overlap) return;            // CN_NO_OVERLAP: no copy stream, no side streams: the load does it all
        require_targets("cn_fraction_prefetch_resident", post_output, f);
        cn_ctx::Prefetch &pf = ctx->pf;
        if (pf.valid && pf.launched) throw cn_error(CN_ERR_STATE, "cn_fraction_prefetch_resident: the previous prefetch has not been consumed by a cn_fraction_load_resident yet");
        if (!pf.allocated) {          // the alternates of the four buffers a fraction is re-laid out into (same initial contents)
            const size_t maxN = input->maxN(), guard = (size_t)CN_GUARD_STEPS * ctx->PSp;
            HIP_CHECK(hipMalloc((void **)&pf.pat_raw, cn_ctx::pat_bytes(maxN, guard)));
            HIP_CHECK(hipMemsetAsync(pf.pat_raw, 0, cn_ctx::pat_bytes(maxN, guard), ctx->stream));
            pf.pat = pf.pat_raw + guard;
            HIP_CHECK(hipMalloc((void **)&pf.tcls, maxN * sizeof(int)));
            HIP_CHECK(hipMemsetAsync(pf.tcls, 0xFF, maxN * sizeof(int), ctx->stream));
            pf.in_op = dalloc(input, maxN * input->Lp * ctx->esz());
            if (post_output && post_output->targets) pf.targets = (float *)dalloc(post_output, maxN * post_output->size * sizeof(float));
            pf.allocated = true;
        }
        if (post_output && post_output->targets && !pf.targets) pf.targets = (float *)dalloc(post_output, input->maxN() * post_output->size * sizeof(float));
        check_augment_shape(ctx->aug, ctx->splice, input);
        pf.f = *f; pf.input = input; pf.post = post_output; pf.launched = false; pf.host = host;
        pf.aug = ctx->aug;                  // the load that follows is a hit only under these settings
        pf.splice = ctx->splice;
        if (aug_enabled(pf.aug) || splice_enabled(pf.splice)) ensure_aug_table(ctx, pf.aug_tab);
        if (host) {
            // pack and upload NOW (copy stream, beside whatever the device is doing); the re-layout follows on the side stream of the
            // next gradient work, reading the staging area
            const Staged sg = stage_upload(ctx, input, post_output, f);
            pf.f_host = *f; pf.slot = sg.slot; pf.f = sg.f;
        }
        pf.valid = true;
    });
}

// ---------------------------------------------------------------------------------------------
// forward / backward / loss
// ---------------------------------------------------------------------------------------------
static int post_kind(const cn_layer *l)
{
    switch (l->kind) {
    case CN_LAYER_WEIGHTEDSSE:           return POST_WEIGHTEDSSE;
    case CN_LAYER_SSE_MASK:              return POST_SSE_MASK;
    case CN_LAYER_CE:                    return POST_CE;
    case CN_LAYER_RMSE:                  return POST_RMSE;
    case CN_LAYER_BINARY_CLASSIFICATION: return POST_BINARY;
    default:                             return POST_SSE;
    }
}

// ---- CTC (cn_ctc.hip) ---------------------------------------------------------------------------
// Host side of a label set: per slot the offsets, per label the chain of later occurrences of the same label in its sequence
// buf: [labels | next | first] of `stride` ints each, then laboff [PSp + 1] (CtcArgs); returns 2 * (longest sequence) + 1
static int ctc_pack_labels(int *buf, const int *labels, const int *lengths, int num_sequences, int PSp, size_t stride, int C)
{
    int *lab = buf, *next = lab + stride, *first = next + stride, *off = first + stride;
    std::vector<int> last(C, -1);                 // position of the label's latest occurrence in the current sequence
    int pos = 0, maxS = 1;
    for (int s = 0; s < PSp; ++s) {
        off[s] = pos;
        const int U = s < num_sequences ? lengths[s] : 0;
        for (int u = 0; u < U; ++u) {
            const int k = labels[pos + u], v = last[k];
            lab[pos + u] = k; next[pos + u] = -1; first[pos + u] = v < 0;
            if (v >= 0) next[pos + v] = u;
            last[k] = u;
        }
        for (int u = 0; u < U; ++u) last[labels[pos + u]] = -1;
        maxS = std::max(maxS, 2 * U + 1);
        pos += U;
    }
    off[PSp] = pos;
    return maxS;
}
static CtcArgs ctc_args(cn_layer *post)
{
    cn_ctx *c = post->ctx;
    cn_layer *o = post->prev;
    const size_t stride = post->ctc_stride;
    CtcArgs a{};
    a.y = posteriors(o); a.pat = post->ax->pat; a.T = post->ax->T; a.PSp = c->PSp; a.C = post->size; a.Lp = o->Lp;
    a.labels = post->ctc_labels; a.next = a.labels + stride; a.first = a.next + stride; a.laboff = a.first + stride;
    a.maxS = post->ctc_maxS; a.alpha = post->ctc_alpha; a.beta = post->ctc_beta; a.Sp = round_up(post->ctc_maxS, 64);
    a.info = post->ctc_info; a.rowstat = post->ctc_rowstat; a.err = o->err;
    return a;
}
// the sweeps of the current forward pass: enqueued by whoever needs them first (the error or the output errors), once
static CtcArgs ctc_swept(cn_layer *post, const char *who)
{
    if (!post->ctc_labels_valid)
        throw cn_error(CN_ERR_STATE, std::string(who) + ": the ctc layer has no label sequences for the loaded fraction (call cn_layer_set_label_sequences after cn_fraction_load)");
    const CtcArgs a = ctc_args(post);
    if (!post->ctc_swept) { launch_ctc_sweeps(post->ctx->stream, a); post->ctc_swept = true; }
    return a;
}

int cn_layer_forward(cn_layer *layer)
{
    if (!layer) { g_last_error = "cn_layer_forward: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(layer->ctx);
        require_loaded(layer->ctx);
        finalize(layer->ctx);
        join_side(layer->ctx);
        if (layer->cx_stride == 1) require_axis(layer, "cn_layer_forward");     // (a strided layer forms its own, from its predecessor's)
        if (layer->trainable && !takes_err(layer->prev) && opt().noise_ahead) noise_ahead(layer->ctx);
        if (layer->lstm) lstm_forward(layer);
        else if (layer->trainable) ff_forward(layer);
        else if (layer->context) context_forward(layer);
        /* input and post output layers: no-op (InputLayer.cpp:62-65, SsePostOutputLayer.cu:134-137) */
    });
}

int cn_layer_backward(cn_layer *layer)
{
    if (!layer) { g_last_error = "cn_layer_backward: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        refuse_swapped(c, "cn_layer_backward");
        require_loaded(c);
        finalize(c);
        require_axis(layer, "cn_layer_backward");
        if (layer->trainable && layer->updated)
            throw cn_error(CN_ERR_STATE, c->arm.adam
                ? "cn_layer_backward: the armed update of this layer's previous backward pass has not been completed (call cn_adam_update_all / cn_adam_update first)"
                : "cn_layer_backward: the armed update of this layer's previous backward pass has not been completed (call cn_sgd_update_all / cn_sgd_update first)");
        if (layer->trainable) c->clip_valid = false;        // (the gradient changes: the next update call forms its norm)
        if (layer->lstm) lstm_backward(layer);
        else if (layer->trainable) ff_backward(layer);
        else if (layer->context) context_backward(layer);
        else if (layer->post) {
            Timed tm(c, KC_OTHER);
            cn_layer *o = layer->prev;
            if (layer->kind == CN_LAYER_MULTICLASS_CLASSIFICATION)
                o->mcc_pending = true;         // injected inside the output layer's backward pass (fused kernel)
            else if (layer->kind == CN_LAYER_CTC)
                launch_ctc_errors(c->stream, ctc_swept(layer, "cn_layer_backward"));
            else
                launch_post_backward(c->stream, post_kind(layer), posteriors(o), post_targets(layer), layer->ax->pat, layer->ax->N, o->size, o->Lp, o->err);
        }
    });
}

// The current fraction's error and correct count into dst[2]: overwritten (per_call, cn_loss_eval) or added to (cn_loss_accumulate)
static void launch_loss(cn_layer *post, float *dst, bool per_call)
{
    cn_ctx *c = post->ctx;
    cn_layer *o = post->prev;
    const TimeAxis *ax = post->ax;
    require_axis(post, per_call ? "cn_loss_eval" : "cn_loss_accumulate");
    if (post->kind == CN_LAYER_MULTICLASS_CLASSIFICATION && c->rowstat_of == o) {      // the softmax forward pass left the row statistics
        launch_rowstat_reduce(c->stream, c->d_rowstat, ax->N, dst, per_call);
        return;
    }
    if (post->kind == CN_LAYER_CTC) {                                                   // its own rows: -log p in the row of t = 0 of every slot
        const CtcArgs a = ctc_swept(post, per_call ? "cn_loss_eval" : "cn_loss_accumulate");
        launch_rowstat_reduce(c->stream, a.rowstat, c->PSp, dst, per_call, 1.0f);
        return;
    }
    flush_loss(c);                     // (the row statistics are about to be overwritten)
    if (post->kind == CN_LAYER_MULTICLASS_CLASSIFICATION)
        launch_mcc_eval(c->stream, posteriors(o), ax->tcls, ax->N, post->size, o->Lp, dst, per_call, c->d_rowstat);
    else
        launch_post_eval(c->stream, post_kind(post), posteriors(o), post_targets(post), ax->pat, ax->N, o->size, o->Lp, c->d_rowstat, dst, per_call);
    c->rowstat_of = nullptr;           // the row statistics now are this evaluation's terms
}
// {error, #correct as int bits} at `src` to the host; reset: the running sums are cleared behind the read
static void read_loss_sums(cn_ctx *c, const float *src, bool reset, float *err, int *correct)
{
    float h[2];
    HIP_CHECK(hipMemcpyAsync(h, src, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    if (reset) HIP_CHECK(hipMemsetAsync(c->d_loss_acc, 0, sizeof(h), c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    check_fault(c);
    *err = h[0];
    memcpy(correct, &h[1], sizeof(int));
}

int cn_loss_eval(cn_layer *post, float *error, int *correct)
{
    if (!post || !error) { g_last_error = "cn_loss_eval: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = post->ctx;
        enter(c);
        if (!post->post) throw cn_error(CN_ERR_BAD_ARG, "cn_loss_eval: not a post output layer");
        require_loaded(c);
        {
            Timed tm(c, KC_OTHER);
            launch_loss(post, c->d_loss, true);
        }
        int cc = 0;
        read_loss_sums(c, c->d_loss, false, error, &cc);
        if (correct) *correct = (is_class_post(post) || post->kind == CN_LAYER_CTC) ? cc : -1;
    });
}

int cn_loss_accumulate(cn_layer *post)
{
    if (!post) { g_last_error = "cn_loss_accumulate: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = post->ctx;
        enter(c);
        if (!post->post) throw cn_error(CN_ERR_BAD_ARG, "cn_loss_accumulate: not a post output layer");
        require_loaded(c);
        cn_layer *o = post->prev;
        require_axis(post, "cn_loss_accumulate");
        flush_loss(c);
        // Training: the backward pass of the output layer follows; its launch (softmax_mcc_bwd_kernel) takes the sum along in one
        // extra workgroup, so nothing is enqueued here.  Whoever needs the sums or overwrites the rows first flushes (flush_loss).
        const bool defer_off = opt().no_loss_defer;
        if (post->kind == CN_LAYER_MULTICLASS_CLASSIFICATION && c->rowstat_of == o && !c->timing && !defer_off && softmax_mcc_bwd_takes_loss(o->Lp)) {
            c->loss_deferred = true;
            return;
        }
        Timed tm(c, KC_OTHER);
        launch_loss(post, c->d_loss_acc, false);       // (nothing is deferred any more: its flush_loss does nothing)
    });
}

int cn_layer_set_label_sequences(cn_layer *ctc, const int *labels, const int *label_lengths, int num_sequences)
{
    if (!ctc || (!label_lengths && num_sequences > 0)) { g_last_error = "cn_layer_set_label_sequences: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = ctc->ctx;
        enter(c);
        if (ctc->kind != CN_LAYER_CTC) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_label_sequences: not a ctc layer");
        require_loaded(c);
        if (num_sequences != c->numSeqs)
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_label_sequences: " + std::to_string(num_sequences) + " label sequences for a fraction of " +
                                           std::to_string(c->numSeqs) + " sequences");
        size_t total = 0;
        for (int s = 0; s < num_sequences; ++s) {
            if (label_lengths[s] < 0) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_label_sequences: negative label sequence length");
            if (label_lengths[s] > ctc->ctc_cap)
                throw cn_error(CN_ERR_SHAPE, "cn_layer_set_label_sequences: a label sequence of " + std::to_string(label_lengths[s]) +
                                             " labels exceeds this layer's cap of " + std::to_string(ctc->ctc_cap) +
                                             " (set the context option ctc_max_labels before the layer is created)");
            total += (size_t)label_lengths[s];
        }
        if (total && !labels) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_label_sequences: labels missing");
        for (size_t i = 0; i < total; ++i)
            if (labels[i] < 0 || labels[i] > ctc->size - 2)
                throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_label_sequences: label " + std::to_string(labels[i]) + " outside [0, " +
                                               std::to_string(ctc->size - 2) + "] (the last unit is the blank)");
        // packed with the fraction's own label total as the stride: what is uploaded is what is used
        const size_t stride = std::max<size_t>(total, 1), ints = 3 * stride + c->PSp + 1;
        const unsigned b = ctc->ctc_uploads++ & 1u;
        if (!ctc->ctc_hbuf[b]) {
            HIP_CHECK(hipHostMalloc((void **)&ctc->ctc_hbuf[b], (3 * (size_t)ctc->ctc_cap * ctc->PS + c->PSp + 1) * sizeof(int), hipHostMallocDefault));
            HIP_CHECK(hipEventCreateWithFlags(&ctc->ctc_ev[b], hipEventDisableTiming));
        } else HIP_CHECK(hipEventSynchronize(ctc->ctc_ev[b]));        // the upload two fractions ago has read this image
        ctc->ctc_maxS = ctc_pack_labels(ctc->ctc_hbuf[b], labels, label_lengths, num_sequences, c->PSp, stride, ctc->size);
        ctc->ctc_stride = stride;
        HIP_CHECK(hipMemcpyAsync(ctc->ctc_labels, ctc->ctc_hbuf[b], ints * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipEventRecord(ctc->ctc_ev[b], c->stream));
        ctc->ctc_labels_valid = true; ctc->ctc_swept = false;
    });
}

int cn_loss_read(cn_ctx *ctx, float *error_sum, int64_t *correct_sum, int reset)
{
    if (!ctx) { g_last_error = "cn_loss_read: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        flush_loss(ctx);
        float err = 0.f; int cc = 0;
        read_loss_sums(ctx, ctx->d_loss_acc, reset != 0, &err, &cc);
        if (error_sum) *error_sum = err;
        if (correct_sum) *correct_sum = cc;
    });
}

// ---- CTC decoding (cn_ctc_decode.hip) ------------------------------------------------------------
static unsigned long long *ctc_sums(cn_ctx *c)
{
    if (!c->d_ctc_sums) {
        HIP_CHECK(hipMalloc((void **)&c->d_ctc_sums, 2 * sizeof(unsigned long long)));
        HIP_CHECK(hipMemsetAsync(c->d_ctc_sums, 0, 2 * sizeof(unsigned long long), c->stream));
    }
    return c->d_ctc_sums;
}
// The launches on the posteriors of the current forward pass; sums: the context's running sums take the fraction's numbers
static CtcDecodeArgs ctc_decode_launch(cn_layer *post, const char *who, bool sums)
{
    cn_ctx *c = post->ctx;
    if (post->kind != CN_LAYER_CTC) throw cn_error(CN_ERR_BAD_ARG, std::string(who) + ": not a ctc layer");
    require_loaded(c);
    cn_layer *o = post->prev;
    require_axis(post, who);
    if (o->fwd_serial != c->frac_serial)
        throw cn_error(CN_ERR_STATE, std::string(who) + ": the softmax layer in front of the ctc layer has no forward pass of the current fraction");
    if (sums && !post->ctc_labels_valid)
        throw cn_error(CN_ERR_STATE, std::string(who) + ": the ctc layer has no label sequences for the loaded fraction (call cn_layer_set_label_sequences after cn_fraction_load)");
    const TimeAxis *ax = post->ax;
    const int maxU = post->ctc_labels_valid ? (post->ctc_maxS - 1) / 2 : 0;
    if (!ctc_decode_fits(ax->T, maxU))
        throw cn_error(CN_ERR_SHAPE, std::string(who) + ": min(steps, longest label sequence) = " + std::to_string(std::min(ax->T, maxU)) +
                                     " exceeds " + std::to_string(CTC_DECODE_MAX_SHORT) + " (the distance's three diagonals in LDS)");
    const size_t maxN = post->maxN();
    if (!post->ctc_dec) post->ctc_dec = (int *)dalloc(post, (2 * maxN + 2 * (size_t)c->PSp) * sizeof(int));
    CtcDecodeArgs a{};
    a.pat = ax->pat; a.T = ax->T; a.PSp = c->PSp; a.C = post->size;
    int *amax = post->ctc_dec;
    a.amax = amax; a.decoded = amax + maxN; a.decoded_len = a.decoded + maxN; a.dist = a.decoded_len + c->PSp;
    if (post->ctc_labels_valid) { a.labels = post->ctc_labels; a.laboff = post->ctc_labels + 3 * post->ctc_stride; }
    a.maxShort = std::min(ax->T, maxU);
    a.sums = sums ? ctc_sums(c) : nullptr;
    Timed tm(c, KC_OTHER);
    launch_ctc_argmax(c->stream, posteriors(o), ax->pat, ax->N, post->size, o->Lp, amax);
    if (!opt().ctc_decode_argmax_only) launch_ctc_collapse(c->stream, a);
    return a;
}

int cn_ctc_decode(cn_layer *ctc, int *decoded, int *decoded_lengths, int *distances)
{
    if (!ctc) { g_last_error = "cn_ctc_decode: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = ctc->ctx;
        enter(c);
        const CtcDecodeArgs a = ctc_decode_launch(ctc, "cn_ctc_decode", false);
        const size_t S = (size_t)c->numSeqs;
        if (decoded && S) HIP_CHECK(hipMemcpyAsync(decoded, a.decoded, S * a.T * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (decoded_lengths && S) HIP_CHECK(hipMemcpyAsync(decoded_lengths, a.decoded_len, S * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (distances && S) HIP_CHECK(hipMemcpyAsync(distances, a.dist, S * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        check_fault(c);
    });
}

int cn_ctc_decode_accumulate(cn_layer *ctc)
{
    if (!ctc) { g_last_error = "cn_ctc_decode_accumulate: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctc->ctx);
        ctc_decode_launch(ctc, "cn_ctc_decode_accumulate", true);
    });
}

int cn_ctc_decode_read(cn_ctx *ctx, int64_t *label_errors, int64_t *labels, int reset)
{
    if (!ctx) { g_last_error = "cn_ctc_decode_read: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        unsigned long long h[2] = {0, 0};
        if (ctx->d_ctc_sums) {                 // (no decoding call yet: the sums are 0)
            HIP_CHECK(hipMemcpyAsync(h, ctx->d_ctc_sums, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
            if (reset) HIP_CHECK(hipMemsetAsync(ctx->d_ctc_sums, 0, sizeof(h), ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            check_fault(ctx);
        }
        if (label_errors) *label_errors = (int64_t)h[0];
        if (labels) *labels = (int64_t)h[1];
    });
}

int cn_loss_read_global(cn_ctx *ctx, float *error_sum, int64_t *correct_sum, int reset)
{
    if (!ctx) { g_last_error = "cn_loss_read_global: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        require_comm(ctx, "cn_loss_read_global");
        enter(ctx);
        flush_loss(ctx);
        float err = 0.f; int cc = 0;
        if (ctx->ipc) {          // this rank's sums to the host, added across the ranks there
            read_loss_sums(ctx, ctx->d_loss_acc, reset != 0, &err, &cc);
            try { ipc_comm_check(ctx->ipc, ctx->comm_stream); ipc_allreduce_loss(ctx->ipc, &err, &cc); }
            catch (const std::exception &e) { ipc_comm_mark_failed(ctx->ipc); throw cn_error(CN_ERR_COMM, e.what()); }
        } else {                 // added across the ranks on the device
            float *g = ctx->d_loss + 4;
            RCCL_CHECK(rccl().GroupStart());
            RCCL_CHECK(rccl().AllReduce(ctx->d_loss_acc, g, 1, ncclFloat32, ncclSum, ctx->comm, ctx->stream));
            RCCL_CHECK(rccl().AllReduce(ctx->d_loss_acc + 1, g + 1, 1, ncclInt32, ncclSum, ctx->comm, ctx->stream));
            RCCL_CHECK(rccl().GroupEnd());
            read_loss_sums(ctx, g, reset != 0, &err, &cc);
        }
        if (error_sum) *error_sum = err;
        if (correct_sum) *correct_sum = cc;
    });
}

// ---------------------------------------------------------------------------------------------
// weights and buffers
// ---------------------------------------------------------------------------------------------
int cn_layer_set_weights(cn_layer *layer, const float *host, int count)
{
    if (!layer || !host) { g_last_error = "cn_layer_set_weights: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_weights: layer has no weights");
        refuse_swapped(c, "cn_layer_set_weights");
        if (count != layer->nw)
            throw cn_error(CN_ERR_SHAPE, "Invalid number of weights: " + std::to_string(count) + " given, " + std::to_string(layer->nw) + " expected");
        if (!c->finalized) { layer->pending_w.assign(host, host + count); return; }
        HIP_CHECK(hipMemcpyAsync(layer->w, host, (size_t)count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        layer->dirty = true; layer->noisy_ready = false;
    });
}

int cn_layer_upload(cn_layer *layer, cn_buffer which, const float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_layer_upload: NULL argument"; return CN_ERR_BAD_ARG; }
    if (which == CN_BUF_WEIGHTS) return cn_layer_set_weights(layer, host, (int)count);
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_upload: layer has no weights");
        refuse_swapped(c, "cn_layer_upload");
        if (which != CN_BUF_WEIGHT_UPDATES && which != CN_BUF_WEIGHT_DELTAS && which != CN_BUF_ADAM_SECOND_MOMENTS) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_upload: not a parameter vector");
        if (count != (size_t)layer->nw) throw cn_error(CN_ERR_SHAPE, "cn_layer_upload: count != weight count");
        finalize(c);
        join_side(c);
        if (which == CN_BUF_ADAM_SECOND_MOMENTS) ensure_adam_v(c);
        if (which == CN_BUF_WEIGHT_UPDATES) c->clip_valid = false;
        HIP_CHECK(hipMemcpyAsync(which == CN_BUF_ADAM_SECOND_MOMENTS ? c->adam_v + layer->woff : which == CN_BUF_WEIGHT_UPDATES ? layer->wu : layer->wd, host, count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int cn_layer_write_output_errors(cn_layer *layer, const float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_layer_write_output_errors: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        if (!layer->err) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_write_output_errors: layer has no outputErrors");
        require_axis(layer, "cn_layer_write_output_errors");
        const TimeAxis *ax = layer->ax;
        if (count != (size_t)ax->Next * layer->size) throw cn_error(CN_ERR_SHAPE, "cn_layer_write_output_errors: count != T*PS*size");
        const Scratch scratch(count * sizeof(float));
        float *tmp = scratch.get();
        HIP_CHECK(hipMemcpyAsync(tmp, host, count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        layer->mcc_pending = false;
        layer->err_in_delta = false;
        HIP_CHECK(hipMemsetAsync(layer->err, 0, (size_t)ax->N * layer->Lp * sizeof(float), c->stream));
        launch_pad_f32(c->stream, tmp, ax->Next, layer->err, unit_map(layer), c->PS, c->PSp);
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int cn_layer_read(cn_layer *layer, cn_buffer which, int dir, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_layer_read: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        finalize(c);
        join_side(c);
        const bool opbf = !c->f32;
        // flat parameter vectors
        if (which == CN_BUF_WEIGHTS || which == CN_BUF_WEIGHT_UPDATES || which == CN_BUF_WEIGHT_DELTAS || which == CN_BUF_ADAM_SECOND_MOMENTS) {
            if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: layer has no weights");
            if (count != (size_t)layer->nw) throw cn_error(CN_ERR_SHAPE, "cn_layer_read: count != weight count");
            if (which == CN_BUF_ADAM_SECOND_MOMENTS) {
                if (!c->adam_v) { std::fill(host, host + count, 0.f); return; }          // before any Adam call: what it will start from
                HIP_CHECK(hipMemcpyAsync(host, c->adam_v + layer->woff, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
                HIP_CHECK(hipStreamSynchronize(c->stream));
                return;
            }
            const float *src = which == CN_BUF_WEIGHTS ? layer->w : (which == CN_BUF_WEIGHT_UPDATES ? layer->wu : layer->wd);
            HIP_CHECK(hipMemcpyAsync(host, src, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            return;
        }
        require_loaded(c);
        require_axis(layer, "cn_layer_read");
        const int N = layer->ax->Next;         // host layout: T*PS patterns of the layer's own time axis
        int width = layer->size;
        if (which >= CN_BUF_LSTM_CELL_STATES) {
            if (!layer->lstm) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: not an LSTM layer");
            if (dir < 0 || dir >= layer->dirs) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: direction out of range");
            width = layer->H;
        }
        if (count != (size_t)N * width) throw cn_error(CN_ERR_SHAPE, "cn_layer_read: count != T*PS*width");
        if (which == CN_BUF_OUTPUTS) {
            // what the followers read (bf16 mode: rounded to bf16; a marked layer: its sum); of a dense trainable layer that
            // did not sum, its fp32 outputs
            if (layer->kind == CN_LAYER_INPUT || layer->lstm || layer->summed || layer->context)
                read_rows(c, follower_operand(layer), opbf, unit_map(layer), N, c->PS, c->PSp, host);
            else if (layer->trainable) read_rows(c, posteriors(layer), false, unit_map(layer), N, c->PS, c->PSp, host);
            else throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: layer has no outputs");
            return;
        }
        if (which == CN_BUF_OUTPUT_ERRORS) {
            if (!layer->err) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: layer has no outputErrors");
            if (layer->mcc_pending) {     // the deferred multiclass error injection becomes visible here
                launch_mcc_backward(c->stream, posteriors(layer), layer->ax->tcls, layer->ax->N, layer->size, layer->Lp, layer->err);
                layer->mcc_pending = false;
            }
            const bool in_delta = !layer->lstm && layer->err_in_delta;      // fused softmax backward in bf16 mode: only the operand copy exists
            read_rows(c, in_delta ? layer->delta_op : (const void *)layer->err, in_delta, unit_map(layer), N, c->PS, c->PSp, host);
            return;
        }
        const Scratch scratch(count * sizeof(float));
        float *tmp = scratch.get();
        const int R = layer->dirs * 4 * layer->Hp, Hp = layer->Hp, H = layer->H;
        switch (which) {
        case CN_BUF_LSTM_CELL_STATES:
            launch_unpad(c->stream, false, layer->cell, layer->Lp, dir * Hp, 1, N, H, tmp, H, 0, c->PS, c->PSp); break;
        case CN_BUF_LSTM_TMP_OUTPUTS:
            launch_unpad(c->stream, opbf, layer->out_op, layer->Lp, dir * Hp, 1, N, H, tmp, H, 0, c->PS, c->PSp); break;
        case CN_BUF_LSTM_NI_ACTS: case CN_BUF_LSTM_IG_ACTS: case CN_BUF_LSTM_FG_ACTS: case CN_BUF_LSTM_OG_ACTS:
            launch_unpad(c->stream, false, layer->acts, R, dir * 4 * Hp + (which - CN_BUF_LSTM_NI_ACTS), 4, N, H, tmp, H, 0, c->PS, c->PSp); break;
        case CN_BUF_LSTM_NI_DELTAS: case CN_BUF_LSTM_IG_DELTAS: case CN_BUF_LSTM_FG_DELTAS: case CN_BUF_LSTM_OG_DELTAS:
            launch_unpad(c->stream, opbf, layer->delta_op, R, dir * 4 * Hp + (which - CN_BUF_LSTM_NI_DELTAS), 4, N, H, tmp, H, 0, c->PS, c->PSp); break;
        default:
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read: unknown buffer");
        }
        HIP_CHECK(hipMemcpyAsync(host, tmp, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

void *cn_layer_device_ptr(cn_layer *layer, cn_buffer which)
{
    if (!layer || !layer->trainable) return nullptr;
    if (guarded([&] { enter(layer->ctx); finalize(layer->ctx); }) != CN_OK) return nullptr;
    switch (which) {
    case CN_BUF_WEIGHTS: return layer->w;
    case CN_BUF_WEIGHT_UPDATES: return layer->wu;
    case CN_BUF_WEIGHT_DELTAS: return layer->wd;
    case CN_BUF_ADAM_SECOND_MOMENTS:
        if (guarded([&] { ensure_adam_v(layer->ctx); }) != CN_OK) return nullptr;
        return layer->ctx->adam_v + layer->woff;
    default: return nullptr;
    }
}

int cn_ctx_param_arena(cn_ctx *ctx, void **weights, void **weight_updates, void **weight_deltas, size_t *count)
{
    if (!ctx) { g_last_error = "cn_ctx_param_arena: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        finalize(ctx);
        if (weights) *weights = ctx->arena;
        if (weight_updates) *weight_updates = ctx->arena + ctx->total;
        if (weight_deltas) *weight_deltas = ctx->arena + 2 * ctx->total;
        if (count) *count = ctx->total;
    });
}

int cn_ctx_weights_touched(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_weights_touched: ctx is NULL"; return CN_ERR_BAD_ARG; }
    for (cn_layer *l : ctx->layers) if (l->trainable) { l->dirty = true; l->noisy_ready = false; }
    return CN_OK;
}

// ---- weight averaging (include/currennt_hip.h, section Weight averaging) ----
// the average's allocation (the caller fills it: the first step copies, the first upload copies and overwrites a part)
static float *alloc_avg(cn_ctx *c)
{
    float *p = nullptr;
    HIP_CHECK(hipMalloc((void **)&p, (c->total ? c->total : 4) * sizeof(float)));
    return p;
}

int cn_ctx_average_weights(cn_ctx *ctx, float decay)
{
    if (!ctx) { g_last_error = "cn_ctx_average_weights: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (!(decay >= 0.f && decay < 1.f)) throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_average_weights: decay must lie in [0, 1)");
        refuse_swapped(ctx, "cn_ctx_average_weights");
        finalize(ctx);
        join_side(ctx);                      // (the step only reads the weights, but an armed step's updates ran on the side streams)
        const float omd = (float)(1.0 - (double)decay);
        const bool first = !ctx->avg;
        if (first) ctx->avg = alloc_avg(ctx);
        Timed tm(ctx, KC_OTHER);
        launch_weight_average(ctx->stream, ctx->avg, ctx->arena, ctx->total, omd, first || omd == 1.0f);
    });
}

int cn_ctx_swap_weight_average(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_swap_weight_average: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (!ctx->avg) throw cn_error(CN_ERR_STATE, "cn_ctx_swap_weight_average: there is no average yet (cn_ctx_average_weights / cn_layer_upload_weight_average)");
        bool pending = ctx->armed || ctx->arm_deferred;
        for (cn_layer *l : ctx->layers) pending = pending || l->updated || l->deferred;
        if (pending) throw cn_error(CN_ERR_STATE, "cn_ctx_swap_weight_average: an armed update is pending (complete it with the *_update* call first)");
        join_side(ctx);
        // the swap WRITES the flat weights: behind the launches that still read them elsewhere -- the operand copies an update left
        // on the side stream (one wait, for the last of them: same stream, in order), noisy sets generated ahead
        bool packs = false;
        for (cn_layer *l : ctx->layers) { packs = packs || l->pack_pending; l->pack_pending = false; }
        if (packs && ctx->ev_pack_last) HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_pack_last, 0));
        if (ctx->noise_wait) { HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_noise, 0)); ctx->noise_wait = false; }
        {
            Timed tm(ctx, KC_OTHER);
            launch_weight_swap(ctx->stream, ctx->arena, ctx->avg, ctx->total);
        }
        ctx->avg_swapped = !ctx->avg_swapped;
        // every copy of the old weights is stale: the next forward pass rebuilds them all, a noisy backward pass its sets
        for (cn_layer *l : ctx->layers) if (l->trainable) { l->dirty = true; l->noisy_ready = false; }
    });
}

int cn_ctx_weight_average_state(const cn_ctx *ctx, int *exists, int *swapped)
{
    if (!ctx) { g_last_error = "cn_ctx_weight_average_state: ctx is NULL"; return CN_ERR_BAD_ARG; }
    if (exists) *exists = ctx->avg ? 1 : 0;
    if (swapped) *swapped = ctx->avg_swapped ? 1 : 0;
    return CN_OK;
}

int cn_layer_read_weight_average(cn_layer *layer, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_layer_read_weight_average: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_read_weight_average: layer has no weights");
        if (count != (size_t)layer->nw) throw cn_error(CN_ERR_SHAPE, "cn_layer_read_weight_average: count != weight count");
        finalize(c);
        join_side(c);
        const float *src = c->avg ? c->avg + layer->woff : layer->w;       // before an average exists: what the first step will copy
        HIP_CHECK(hipMemcpyAsync(host, src, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int cn_layer_upload_weight_average(cn_layer *layer, const float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_layer_upload_weight_average: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_upload_weight_average: layer has no weights");
        refuse_swapped(c, "cn_layer_upload_weight_average");
        if (count != (size_t)layer->nw) throw cn_error(CN_ERR_SHAPE, "cn_layer_upload_weight_average: count != weight count");
        finalize(c);
        join_side(c);
        if (!c->avg) {                       // the average starts as a copy of all weights
            c->avg = alloc_avg(c);
            HIP_CHECK(hipMemcpyAsync(c->avg, c->arena, c->total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_CHECK(hipMemcpyAsync(c->avg + layer->woff, host, count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

// ---- the optimizer's calls: momentum SGD and Adam share every sequence, the rule says which -------------------------
static UpdateRule sgd_rule(float lr, float mom) { UpdateRule r; r.lr = lr; r.mom = mom; return r; }
static UpdateRule adam_rule(float lr, float b1, float b2, float eps, int64_t step)
{
    UpdateRule r; r.adam = true; r.lr = lr; r.b1 = b1; r.b2 = b2; r.eps = eps; r.step = step;
    return r;
}
static UpdateRule lamb_rule(float lr, float b1, float b2, float eps, int64_t step)
{
    UpdateRule r = adam_rule(lr, b1, b2, eps, step); r.lamb = true;
    return r;
}
// what every update call does first (fn: the ABI function, for the messages); on return the main stream is ordered behind all
// gradient work
static void begin_update(cn_ctx *c, const UpdateRule &r, const char *fn)
{
    refuse_swapped(c, fn);
    if (r.adam) check_adam_args(fn, r);
    bind_family(c, rule_family(r), fn);
    comm_check_fast(c);
    if (r.lamb) ensure_lamb(c); else if (r.adam) ensure_adam_v(c); else finalize(c);
    join_side(c);
}
[[noreturn]] static void throw_rule_mismatch(const char *fn, const UpdateRule &r)
{
    const bool adam = r.adam;
    if (r.lamb) throw cn_error(CN_ERR_STATE, std::string(fn) + ": learning rate / betas / eps / step differ from what cn_ctx_arm_lamb armed");
    throw cn_error(CN_ERR_STATE, std::string(fn) + (adam ? ": learning rate / betas / eps / step differ from what cn_ctx_arm_adam armed and applied"
                                                          : ": learning rate / momentum differ from what cn_ctx_arm_update armed and applied"));
}
// the flat forms: momentum SGD or Adam over a range of the arena that starts `off` floats in, at rate lr
// clip: the record of the step's norm (clip_record below), or null with clipping off
// decayed (with r.decay on; then the range is ONE layer's): the runs of the range that decay (decay_ranges)
static void launch_flat(cn_ctx *c, const UpdateRule &r, size_t off, size_t n, float lr, const ClipRecord *clip, hipEvent_t done = nullptr,
                        const DecayRanges *decayed = nullptr)
{
    if (r.lamb) throw cn_error(CN_ERR_STATE, "launch_flat: LAMB steps go by layers (launch_lamb_layers)");
    if (r.decay != 0.f && !decayed) throw cn_error(CN_ERR_STATE, "launch_flat: weight decay needs a layer's range");
    float *w = c->arena + off;
    const FlatUpdate u{w, w + c->total, w + 2 * c->total, n, lr, r.mom};
    FlatAdam ad{};
    FlatDecay dk{};
    if (r.adam) ad = FlatAdam{c->adam_v + off, adam_scalars(r, lr)};
    if (r.decay != 0.f) dk = FlatDecay{decay_ld(lr, r.decay), *decayed};
    launch_flat_update(c->stream, u, r.adam ? &ad : nullptr, clip, r.decay != 0.f ? &dk : nullptr, done);
}
// Behind begin_update (the main stream is ordered behind the side streams' gradient work and the reductions): the record the
// update launches of this step read, or null with clipping off.  The norm is formed once per gradient: by the first update call
// after the gradient last changed; the per-layer calls that follow reuse the record.
static const ClipRecord *clip_record(cn_ctx *c)
{
    if (c->clip_max == 0.f || !c->total) return nullptr;
    if (!c->clip_valid) {
        launch_grad_norm(c->stream, c->arena + c->total, c->total, c->clip_max, c->clip_rec);
        c->clip_valid = true;
    }
    return c->clip_rec;
}

// LAMB (include/currennt_hip.h, section LAMB): the direction and apply launches over `layers` (all of them in groups of
// LAMB_GROUP_MAX, not one launch pair per layer); own_rates: a layer with a rate of its own takes it (layer_lr), else r.lr is the
// rate as it stands; done rides on the last apply launch
static void launch_lamb_layers(cn_ctx *c, const UpdateRule &r, const std::vector<cn_layer *> &layers, bool own_rates, const ClipRecord *clip, hipEvent_t done = nullptr)
{
    const LambScalars a = lamb_scalars(c, r);
    for (size_t first = 0; first < layers.size(); first += LAMB_GROUP_MAX) {
        LambGroup grp{};
        for (size_t k = first; k < layers.size() && k < first + LAMB_GROUP_MAX; ++k) {
            const cn_layer *l = layers[k];
            const DecayRanges rg = decay_ranges(l);
            LambItem &it = grp.item[grp.n++];
            it.off = l->woff; it.n = (unsigned)round_up(l->nw, 4);
            it.a1 = (unsigned)rg.a1; it.b0 = (unsigned)rg.b0; it.b1 = (unsigned)rg.b1;
            it.lr = own_rates ? layer_lr(l, r) : r.lr; it.rec = l->lamb_rec;
        }
        const bool last = first + LAMB_GROUP_MAX >= layers.size();
        launch_lamb(c->stream, grp, c->arena, c->total, c->adam_v, c->lamb_u, a, c->lamb_recs, clip, last ? done : nullptr);
    }
}

// cn_ctx_arm_update / cn_ctx_arm_adam / cn_ctx_arm_lamb
static void arm(cn_ctx *ctx, UpdateRule r, const char *fn)
{
    enter(ctx);
    r.decay = ctx->decay;              // (the armed step records the decay in force now)
    refuse_swapped(ctx, fn);
    if (r.adam) check_adam_args(fn, r);
    for (cn_layer *l : ctx->layers)
        if (l->updated) throw cn_error(CN_ERR_STATE, std::string(fn) + ": the previous armed update has not been completed (" +
                                       (r.lamb ? "cn_lamb_update_all" : r.adam ? "cn_adam_update_all" : "cn_sgd_update_all") + ")");
    bind_family(ctx, rule_family(r), fn);
    if (r.lamb) ensure_lamb(ctx); else if (r.adam) ensure_adam_v(ctx);
    ctx->arm = r;
    // clipping on: accepted and checked, applied by the completing call (a global norm needs every layer's gradient); LAMB: the
    // same deferral, always (its direction pass writes a layer's moments before the layer's ratio is known)
    if (ctx->clip_max != 0.f || r.lamb) {
        ctx->arm_deferred = true;
        for (cn_layer *l : ctx->layers) l->deferred = l->trainable;
        return;
    }
    ctx->armed = true;
}

int cn_ctx_arm_update(cn_ctx *ctx, float learning_rate, float momentum)
{
    if (!ctx) { g_last_error = "cn_ctx_arm_update: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { arm(ctx, sgd_rule(learning_rate, momentum), "cn_ctx_arm_update"); });
}

int cn_ctx_arm_adam(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!ctx) { g_last_error = "cn_ctx_arm_adam: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { arm(ctx, adam_rule(learning_rate, beta1, beta2, eps, step), "cn_ctx_arm_adam"); });
}

// cn_sgd_update / cn_adam_update: r.lr is the layer's effective rate (the caller applies the layer's own)
static void update_layer(cn_layer *layer, UpdateRule r, const char *fn)
{
    cn_ctx *c = layer->ctx;
    enter(c);
    r.decay = c->decay;
    if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, std::string(fn) + ": layer has no weights");
    begin_update(c, r, fn);
    if (layer->updated) {            // armed: this layer's step ran behind its gradient; nothing left but the wait above
        UpdateRule applied = c->arm;
        applied.lr = layer_lr(layer, c->arm);
        if (!same_rule(r, applied)) throw_rule_mismatch(fn, r);
        layer->updated = false;
        bool any = false;
        for (cn_layer *o : c->layers) any = any || o->updated;
        if (!any) c->armed = false;
        return;
    }
    if (layer->deferred) {           // armed with clipping on: this is the call that applies the layer's step
        UpdateRule armed = c->arm;
        armed.lr = layer_lr(layer, c->arm);
        if (!same_rule(r, armed)) throw_rule_mismatch(fn, r);
        layer->deferred = false;
        r.decay = c->arm.decay;
        bool any = false;
        for (cn_layer *o : c->layers) any = any || o->deferred;
        if (!any) c->arm_deferred = false;
    }
    Timed tm(c, KC_OTHER);
    if (r.lamb) {
        launch_lamb_layers(c, r, {layer}, false, clip_record(c));
        layer->dirty = true; layer->noisy_ready = false;
        return;
    }
    const DecayRanges rg = decay_ranges(layer);
    launch_flat(c, r, layer->woff, (size_t)layer->nw, r.lr, clip_record(c), nullptr, &rg);
    layer->dirty = true; layer->noisy_ready = false;
}

int cn_sgd_update(cn_layer *layer, float learning_rate, float momentum)
{
    if (!layer) { g_last_error = "cn_sgd_update: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_layer(layer, sgd_rule(learning_rate, momentum), "cn_sgd_update"); });
}

int cn_adam_update(cn_layer *layer, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!layer) { g_last_error = "cn_adam_update: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_layer(layer, adam_rule(learning_rate, beta1, beta2, eps, step), "cn_adam_update"); });
}

int cn_ctx_accumulate_updates(cn_ctx *ctx, int first)
{
    if (!ctx) { g_last_error = "cn_ctx_accumulate_updates: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        finalize(ctx);
        refuse_swapped(ctx, "cn_ctx_accumulate_updates");
        if (ctx->armed || ctx->arm_deferred) throw cn_error(CN_ERR_STATE, "cn_ctx_accumulate_updates: an armed per-fraction update is pending (batch learning sums first, cn_ctx_arm_update is not for it)");
        if (!first && !ctx->acc_valid) throw cn_error(CN_ERR_STATE, "cn_ctx_accumulate_updates: nothing accumulated yet (the first fraction of an epoch passes first != 0)");
        join_side(ctx);                     // the gradient GEMMs / unpack launches of the side streams write weightUpdates
        if (!ctx->acc) HIP_CHECK(hipMalloc((void **)&ctx->acc, ctx->total * sizeof(float)));
        Timed tm(ctx, KC_OTHER);
        launch_accumulate(ctx->stream, ctx->acc, ctx->arena + ctx->total, ctx->total, first != 0);
        ctx->acc_valid = true;
    });
}

int cn_ctx_take_accumulated(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_take_accumulated: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        finalize(ctx);
        refuse_swapped(ctx, "cn_ctx_take_accumulated");
        if (!ctx->acc_valid) throw cn_error(CN_ERR_STATE, "cn_ctx_take_accumulated: nothing accumulated (cn_ctx_accumulate_updates)");
        join_side(ctx);
        HIP_CHECK(hipMemcpyAsync(ctx->arena + ctx->total, ctx->acc, ctx->total * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        ctx->clip_valid = false;
        ctx->acc_valid = false;
    });
}

// ---- gradient clipping (include/currennt_hip.h, section Gradient clipping) ----
int cn_ctx_set_grad_clip(cn_ctx *ctx, float max_norm)
{
    if (!ctx) { g_last_error = "cn_ctx_set_grad_clip: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!(max_norm >= 0.f) || std::isinf(max_norm)) throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_set_grad_clip: max_norm must be finite and >= 0 (0 = off)");
        bool pending = ctx->armed || ctx->arm_deferred;
        for (cn_layer *l : ctx->layers) pending = pending || l->updated;
        if (pending) throw cn_error(CN_ERR_STATE, "cn_ctx_set_grad_clip: an armed update is pending (complete it with the *_update* call first)");
        if (max_norm != 0.f && !ctx->clip_rec) {
            enter(ctx);
            HIP_CHECK(hipMalloc((void **)&ctx->clip_rec, sizeof(ClipRecord)));
            HIP_CHECK(hipMemsetAsync(ctx->clip_rec, 0, sizeof(ClipRecord), ctx->stream));
        }
        if (max_norm != ctx->clip_max) ctx->clip_valid = false;       // (the record's factor belongs to the bound it was formed with)
        ctx->clip_max = max_norm;
    });
}

// ---- weight decay (include/currennt_hip.h, section Weight decay) ----
int cn_ctx_set_weight_decay(cn_ctx *ctx, float decay)
{
    if (!ctx) { g_last_error = "cn_ctx_set_weight_decay: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!(decay >= 0.f) || std::isinf(decay)) throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_set_weight_decay: decay must be finite and >= 0 (0 = off)");
        bool pending = ctx->armed || ctx->arm_deferred;
        for (cn_layer *l : ctx->layers) pending = pending || l->updated;
        if (pending) throw cn_error(CN_ERR_STATE, "cn_ctx_set_weight_decay: an armed update is pending (complete it with the *_update* call first)");
        ctx->decay = decay;
    });
}
int cn_ctx_get_weight_decay(const cn_ctx *ctx, float *decay)
{
    if (!ctx || !decay) { g_last_error = "cn_ctx_get_weight_decay: ctx or decay is NULL"; return CN_ERR_BAD_ARG; }
    *decay = ctx->decay;
    return CN_OK;
}

int cn_ctx_grad_clip_stats(cn_ctx *ctx, float *last_norm, float *last_scale, int64_t *updates, int64_t *clipped, int64_t *skipped,
                           float *max_norm_seen, int reset)
{
    if (!ctx) { g_last_error = "cn_ctx_grad_clip_stats: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        ClipRecord h{};
        if (ctx->clip_max != 0.f && ctx->clip_rec) {
            enter(ctx);
            HIP_CHECK(hipMemcpyAsync(&h, ctx->clip_rec, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
            // reset: the counters and the largest norm; the record of the last step stays (a per-layer call may still read it)
            if (reset) HIP_CHECK(hipMemsetAsync((char *)ctx->clip_rec + offsetof(ClipRecord, max_seen), 0,
                                                offsetof(ClipRecord, arrivals) - offsetof(ClipRecord, max_seen), ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        if (last_norm) *last_norm = h.norm;
        if (last_scale) *last_scale = h.scale;
        if (updates) *updates = h.updates;
        if (clipped) *clipped = h.clipped;
        if (skipped) *skipped = h.skipped;
        if (max_norm_seen) *max_norm_seen = h.max_seen;
    });
}

int cn_layer_set_learning_rate(cn_layer *layer, float learning_rate)
{
    if (!layer) { g_last_error = "cn_layer_set_learning_rate: layer is NULL"; return CN_ERR_BAD_ARG; }
    if (!layer->trainable) { g_last_error = "cn_layer_set_learning_rate: layer has no weights"; return CN_ERR_BAD_ARG; }
    layer->own_lr = learning_rate;
    return CN_OK;
}

// ---- residual connections (include/currennt_hip.h, section Residual connections) ----
int cn_layer_set_residual(cn_layer *layer, int enable)
{
    if (!layer) { g_last_error = "cn_layer_set_residual: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        const bool kind_ok = layer->lstm || layer->kind == CN_LAYER_FF_TANH || layer->kind == CN_LAYER_FF_LOGISTIC || layer->kind == CN_LAYER_FF_IDENTITY;
        if (!kind_ok) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_residual: only lstm, blstm and feedforward_* layers can be residual");
        if (layer->size != layer->prev->size)
            throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_residual: a residual layer must have the size of its preceding layer (" +
                                           std::to_string(layer->size) + " vs. " + std::to_string(layer->prev->size) + ")");
        for (const cn_layer *o : layer->ctx->layers)
            if (o->prev == layer && o->post)
                throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_residual: a residual layer directly in front of a post output layer is not supported");
        if (enable && !layer->res_sum) {          // like out_op: same size, cleared once
            enter(layer->ctx);
            layer->res_sum = dalloc(layer, layer->maxN() * layer->Lp * layer->ctx->esz());
            if (!layer->lstm) layer->res_e = (float *)dalloc(layer, layer->maxN() * layer->Lp * sizeof(float));
        }
        layer->residual = enable != 0;
    });
}

int cn_dbg_residual_branch(cn_layer *layer, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_dbg_residual_branch: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        if (!layer->summed) throw cn_error(CN_ERR_STATE, "cn_dbg_residual_branch: the layer's last forward pass did not sum");
        require_axis(layer, "cn_dbg_residual_branch");
        const int N = layer->ax->Next;
        if (count != (size_t)N * layer->size) throw cn_error(CN_ERR_SHAPE, "cn_dbg_residual_branch: count != T*PS*size");
        read_rows(c, layer->out_op, !c->f32, unit_map(layer), N, c->PS, c->PSp, host);
    });
}

// ---- layer normalization (include/currennt_hip.h, section Layer normalization) ----
int cn_layer_set_layer_norm(cn_layer *layer, int enable, float eps)
{
    if (!layer) { g_last_error = "cn_layer_set_layer_norm: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_layer_norm: only lstm, blstm, feedforward_* and softmax layers normalise their input");
        if (layer->P < 2) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_layer_norm: the preceding layer must have at least 2 units");
        if (!std::isfinite(eps) || !(eps > 0.f)) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_layer_norm: eps must be finite and > 0");
        if (enable && !layer->in_norm) {          // like the preceding layer's out_op: same size, cleared once
            enter(layer->ctx);
            layer->in_norm = dalloc(layer, layer->maxN() * layer->Pp * layer->ctx->esz());
            layer->ln_rstd = (float *)dalloc(layer, layer->maxN() * sizeof(float));
        }
        layer->layer_norm = enable != 0;
        layer->ln_eps = eps;
    });
}

int cn_dbg_layer_norm_input(cn_layer *layer, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_dbg_layer_norm_input: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        if (!layer->trainable || !layer->normed) throw cn_error(CN_ERR_STATE, "cn_dbg_layer_norm_input: the layer's last forward pass did not normalise");
        // the geometry of the forward pass that wrote the copy (its record), not of whatever fraction is loaded now
        const LnArgs &a = layer->ln;
        const int frames = a.N / a.PSp * a.PS;
        if (count != (size_t)frames * a.prev.L) throw cn_error(CN_ERR_SHAPE, "cn_dbg_layer_norm_input: count != T*PS*size of the preceding layer (of that forward pass)");
        read_rows(c, layer->in_norm, !c->f32, a.prev, frames, a.PS, a.PSp, host);
    });
}

// ---- dropout (include/currennt_hip.h, section Dropout) ----
int cn_layer_set_dropout(cn_layer *layer, float rate)
{
    if (!layer) { g_last_error = "cn_layer_set_dropout: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_dropout: only lstm, blstm, feedforward_* and softmax layers take dropout on their input");
        if (!(rate >= 0.f && rate < 1.f)) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_set_dropout: the rate must lie in [0, 1)");
        if (rate > 0.f && !layer->in_drop) {      // like the preceding layer's out_op: same size, cleared once
            enter(layer->ctx);
            layer->in_drop = dalloc(layer, layer->maxN() * layer->Pp * layer->ctx->esz());
        }
        layer->drop_rate = rate;
    });
}

int cn_ctx_set_dropout_pass(cn_ctx *ctx, int enable, uint64_t seed, uint64_t pass)
{
    if (!ctx) { g_last_error = "cn_ctx_set_dropout_pass: ctx is NULL"; return CN_ERR_BAD_ARG; }
    ctx->drop_enable = enable != 0; ctx->drop_seed = seed; ctx->drop_pass = pass;
    return CN_OK;
}

int cn_dbg_dropout_input(cn_layer *layer, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_dbg_dropout_input: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        if (!layer->trainable || !layer->dropped) throw cn_error(CN_ERR_STATE, "cn_dbg_dropout_input: the layer's last forward pass did not drop");
        // the geometry of the forward pass that wrote the copy (its record), not of whatever fraction is loaded now
        const DropArgs &a = layer->drop;
        const int frames = a.N / a.PSp * a.PS;
        if (count != (size_t)frames * a.prev.L) throw cn_error(CN_ERR_SHAPE, "cn_dbg_dropout_input: count != T*PS*size of the preceding layer (of that forward pass)");
        read_rows(c, layer->in_drop, !c->f32, a.prev, frames, a.PS, a.PSp, host);
    });
}

// ---- weight noise (include/currennt_hip.h, section Weight noise) ----
int cn_ctx_set_weight_noise(cn_ctx *ctx, float sigma, uint64_t seed, uint64_t pass)
{
    if (!ctx) { g_last_error = "cn_ctx_set_weight_noise: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!(sigma >= 0.f) || std::isinf(sigma)) throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_set_weight_noise: sigma must be finite and >= 0 (0 = off)");
        if (sigma != ctx->noise_sigma || seed != ctx->noise_seed || pass != ctx->noise_pass)
            for (cn_layer *l : ctx->layers) l->noisy_ready = false;      // (sets generated ahead belong to the old triple)
        ctx->noise_sigma = sigma; ctx->noise_seed = seed; ctx->noise_pass = pass;
    });
}

// ---- input augmentation (include/currennt_hip.h, section Input augmentation) ----
int cn_ctx_set_input_augment(cn_ctx *ctx, const cn_input_augment *a)
{
    if (!ctx) { g_last_error = "cn_ctx_set_input_augment: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!a) { ctx->aug = cn_input_augment{}; return; }
        const char *w = "cn_ctx_set_input_augment: ";
        if (!(a->noise_sigma >= 0.f) || std::isinf(a->noise_sigma)) throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "noise_sigma must be finite and >= 0 (0 = no noise)");
        if (a->context_left < 0 || a->context_right < 0) throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "context_left / context_right must be >= 0");
        if (a->freq_masks < 0 || a->freq_masks > AUG_MAX_MASKS || a->time_masks < 0 || a->time_masks > AUG_MAX_MASKS)
            throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "freq_masks / time_masks must be in 0.." + std::to_string(AUG_MAX_MASKS));
        if (a->freq_width < 0 || a->time_width < 0) throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "freq_width / time_width must be >= 0");
        if (a->time_max_permille < 0 || a->time_max_permille > 1000) throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "time_max_permille must be in 0..1000");
        if (!aug_enabled(*a)) { ctx->aug = cn_input_augment{}; return; }      // no noise, no masks: off, whatever the other members say
        enter(ctx);
        ctx->aug = *a;
        ensure_aug_table(ctx, ctx->aug_tab);
    });
}

// ---- input splicing and frame skipping (include/currennt_hip.h, section of that name) ----
int cn_ctx_set_input_splice(cn_ctx *ctx, const cn_input_splice *s)
{
    if (!ctx) { g_last_error = "cn_ctx_set_input_splice: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!s) { ctx->splice = cn_input_splice{}; return; }
        const char *w = "cn_ctx_set_input_splice: ";
        if (s->context_left < 0 || s->context_right < 0 || s->context_left > 32 || s->context_right > 32)
            throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "context_left / context_right must be in 0..32");
        if (s->frame_skip < 1 || s->frame_skip > 16) throw cn_error(CN_ERR_BAD_ARG, std::string(w) + "frame_skip must be in 1..16");
        ctx->splice = *s;
    });
}

int cn_dbg_noisy_weights(cn_layer *layer, float *host, size_t count)
{
    if (!layer || !host) { g_last_error = "cn_dbg_noisy_weights: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        if (!layer->trainable || !layer->noise_used) throw cn_error(CN_ERR_STATE, "cn_dbg_noisy_weights: the layer's last backward pass had no weight noise");
        if (layer->noisy_ready) throw cn_error(CN_ERR_STATE, "cn_dbg_noisy_weights: the noisy copies have been generated again for a pass this layer has not run yet");
        if (count != (size_t)layer->nw) throw cn_error(CN_ERR_SHAPE, "cn_dbg_noisy_weights: count != weight count");
        join_side(c);
        // the copies as floats on the host (bf16 mode: widened there), then the gather in plain C++ (cn_noise_unpack.h)
        auto fetch = [&](const void *dev, size_t n) {
            std::vector<float> out(n);
            if (!n) return out;
            if (c->f32) HIP_CHECK(hipMemcpyAsync(out.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            else {
                std::vector<uint16_t> raw(n);
                HIP_CHECK(hipMemcpyAsync(raw.data(), dev, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
                HIP_CHECK(hipStreamSynchronize(c->stream));
                for (size_t i = 0; i < n; ++i) { const uint32_t b = (uint32_t)raw[i] << 16; memcpy(&out[i], &b, 4); }
            }
            HIP_CHECK(hipStreamSynchronize(c->stream));
            return out;
        };
        NoiseUnpackGeom g{};
        g.lstm = layer->lstm ? 1 : 0; g.L = layer->size; g.Lp = layer->Lp;
        g.dirs = layer->dirs; g.H = layer->H; g.Hp = layer->Hp; g.prev = unit_map(layer->prev);
        const size_t R = (size_t)layer->dirs * 4 * layer->Hp;
        const std::vector<float> WinT = fetch(layer->nWinT, layer->lstm ? R * layer->Pp : (size_t)layer->Lp * layer->Pp);
        std::vector<float> WrecT, peep;
        if (layer->lstm) {
            WrecT = fetch(layer->nWrecT, R * layer->Hp);
            std::vector<float> p((size_t)layer->dirs * 3 * layer->Hp);     // (fp32 in every mode)
            HIP_CHECK(hipMemcpyAsync(p.data(), layer->npeep, p.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
            peep.swap(p);
        }
        std::vector<float> flat(count);
        HIP_CHECK(hipMemcpyAsync(flat.data(), layer->w, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));   // the bias entries
        HIP_CHECK(hipStreamSynchronize(c->stream));
        const size_t bad = noise_unpack(g, WinT, WrecT, peep, flat);
        if (bad) throw cn_error(CN_ERR_STATE, "cn_dbg_noisy_weights: " + std::to_string(bad) + " pad entries of the noisy copies are not exactly 0");
        std::copy(flat.begin(), flat.end(), host);
    });
}

// cn_sgd_update_all / cn_adam_update_all / cn_lamb_update_all: one sequence for all rules (r.lr: the call's learning rate)
// (in an unnamed namespace inside extern "C", as it has been: hipcc gives such a function an unmangled GLOBAL symbol, so the
// library's dynamic symbol table lists "update_all" -- nobody declares it; dropping it is a change of the export list of its own)
namespace {
void update_all(cn_ctx *ctx, UpdateRule r, const char *fn)
{
    enter(ctx);
    r.decay = (ctx->armed || ctx->arm_deferred) ? ctx->arm.decay : ctx->decay;
    begin_update(ctx, r, fn);
    // armed: layers whose step ran behind their gradient are complete (the wait above orders this stream behind them); what
    // follows handles the rest (none, normally)
    bool any_updated = false;
    for (cn_layer *l : ctx->layers) any_updated = any_updated || l->updated;
    if (any_updated && !same_rule(r, ctx->arm)) throw_rule_mismatch(fn, r);
    if (ctx->arm_deferred) {         // armed with clipping on: the step is applied here, all layers at once
        if (!same_rule(r, ctx->arm)) throw_rule_mismatch(fn, r);
        ctx->arm_deferred = false;
        for (cn_layer *l : ctx->layers) l->deferred = false;
    }
    ctx->armed = false;
    struct ClearUpdated { cn_ctx *c; ~ClearUpdated() { for (cn_layer *l : c->layers) l->updated = false; } } clear_updated{ctx};
    Timed tm(ctx, KC_OTHER);
    int ntrain = 0;
    for (cn_layer *l : ctx->layers) if (l->trainable && !l->updated) ++ntrain;
    if (ntrain == 0) return;
    const ClipRecord *clip = clip_record(ctx);
    if (any_updated) {               // some layers were not reached by the armed pass (no backward call for them): one launch each
        for (cn_layer *l : ctx->layers)
            if (l->trainable && !l->updated) launch_layer_update(ctx->stream, l, 1, r, nullptr);
        return;
    }
    // The operand copies of the new weights are rebuilt right away, all layers in ONE launch on this stream
    // (pack_group_kernel): it costs about as much as the first layer's copy alone did, which was on the critical
    // path anyway, and the other layers' copies no longer need a fork event, the side stream and a wait.
    const bool group_off = opt().no_pack_group;
    const bool grouped = ctx->overlap && !group_off && ntrain <= PACK_GROUP_MAX;
    // grouped: the update itself rides on the pack launch (pack_fetch): one kernel instead of two behind the last gradient
    const bool fuse_off = opt().no_sgd_fuse;
    const bool fused = grouped && !fuse_off && !r.lamb;       // (LAMB: its two launches, then the plain pack launch)
    const bool attach = ctx->overlap && !grouped && ctx->attach_forks && !ctx->timing;
    if (ctx->overlap && !grouped && !ctx->ev_sgd) HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_sgd, hipEventDisableTiming));
    if (!fused) {
        bool own_rates = false;
        cn_layer *last = nullptr;
        for (cn_layer *l : ctx->layers)
            if (l->trainable) { own_rates = own_rates || l->own_lr >= 0.f; last = l; }
        if (r.lamb) {
            std::vector<cn_layer *> train;
            for (cn_layer *l : ctx->layers) if (l->trainable) train.push_back(l);
            launch_lamb_layers(ctx, r, train, true, clip, attach ? ctx->ev_sgd : nullptr);
        }
        else if (!own_rates && r.decay == 0.f) launch_flat(ctx, r, 0, ctx->total, r.lr, clip, attach ? ctx->ev_sgd : nullptr);
        else            // a layer with a "learningRate" of its own, or weight decay (a layer's blocks): one launch per layer
            for (cn_layer *l : ctx->layers)
                if (l->trainable) {
                    const DecayRanges rg = decay_ranges(l);
                    launch_flat(ctx, r, l->woff, (size_t)l->nw, layer_lr(l, r), clip, (attach && l == last) ? ctx->ev_sgd : nullptr, &rg);
                }
    }
    for (cn_layer *l : ctx->layers) if (l->trainable) { l->dirty = true; l->noisy_ready = false; }
    if (grouped) {
        PackGroup grp{};
        PackAdam ad{};
        PackDecayArgs dk{};
        for (cn_layer *l : ctx->layers) {
            if (!l->trainable) continue;
            add_pack_item(grp, l);
            if (fused) set_pack_update(grp, ad, dk, 1, r, l);
            l->dirty = false; l->pack_pending = false;
        }
        launch_pack_group(ctx->stream, ctx->f32, grp, nullptr, (fused && r.adam) ? &ad : nullptr, fused ? clip : nullptr,
                          (fused && r.decay != 0.f) ? &dk : nullptr);
    } else if (ctx->overlap) {
        // (more layers than one group launch takes: the first trainable layer's copy on this stream, its forward pass
        // is next; the others on the side stream, each layer's forward pass waits for them in repack())
        if (!attach) HIP_CHECK(hipEventRecord(ctx->ev_sgd, ctx->stream));
        HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->ev_sgd, 0));
        bool first = true;
        for (cn_layer *l : ctx->layers) {
            if (!l->trainable) continue;
            if (first) { first = false; continue; }
            if (!l->ev_pack) HIP_CHECK(hipEventCreateWithFlags(&l->ev_pack, hipEventDisableTiming));
            {
                Timed tp(ctx, KC_OTHER, ctx->side);
                launch_pack(ctx->side, l);
            }
            HIP_CHECK(hipEventRecord(l->ev_pack, ctx->side));
            ctx->ev_pack_last = l->ev_pack;
            l->dirty = false; l->pack_pending = true;
        }
    }
}
}  // namespace

int cn_sgd_update_all(cn_ctx *ctx, float learning_rate, float momentum)
{
    if (!ctx) { g_last_error = "cn_sgd_update_all: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_all(ctx, sgd_rule(learning_rate, momentum), "cn_sgd_update_all"); });
}

int cn_adam_update_all(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!ctx) { g_last_error = "cn_adam_update_all: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_all(ctx, adam_rule(learning_rate, beta1, beta2, eps, step), "cn_adam_update_all"); });
}

// ---- LAMB (include/currennt_hip.h, section LAMB) ----
int cn_lamb_update_all(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!ctx) { g_last_error = "cn_lamb_update_all: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_all(ctx, lamb_rule(learning_rate, beta1, beta2, eps, step), "cn_lamb_update_all"); });
}
int cn_lamb_update(cn_layer *layer, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!layer) { g_last_error = "cn_lamb_update: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { update_layer(layer, lamb_rule(learning_rate, beta1, beta2, eps, step), "cn_lamb_update"); });
}
int cn_ctx_arm_lamb(cn_ctx *ctx, float learning_rate, float beta1, float beta2, float eps, int64_t step)
{
    if (!ctx) { g_last_error = "cn_ctx_arm_lamb: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { arm(ctx, lamb_rule(learning_rate, beta1, beta2, eps, step), "cn_ctx_arm_lamb"); });
}
int cn_ctx_set_trust_bounds(cn_ctx *ctx, float min_ratio, float max_ratio)
{
    if (!ctx) { g_last_error = "cn_ctx_set_trust_bounds: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        if (!(min_ratio >= 0.f) || !(max_ratio >= 0.f) || std::isinf(min_ratio) || std::isinf(max_ratio))
            throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_set_trust_bounds: the bounds must be finite and >= 0 (max_ratio 0 = no upper bound)");
        if (max_ratio != 0.f && min_ratio > max_ratio) throw cn_error(CN_ERR_BAD_ARG, "cn_ctx_set_trust_bounds: min_ratio > max_ratio");
        bool pending = ctx->armed || ctx->arm_deferred;
        for (cn_layer *l : ctx->layers) pending = pending || l->updated;
        if (pending) throw cn_error(CN_ERR_STATE, "cn_ctx_set_trust_bounds: an armed update is pending (complete it with the *_update* call first)");
        ctx->trust_min = min_ratio; ctx->trust_max = max_ratio;
    });
}
int cn_ctx_get_trust_bounds(const cn_ctx *ctx, float *min_ratio, float *max_ratio)
{
    if (!ctx || !min_ratio || !max_ratio) { g_last_error = "cn_ctx_get_trust_bounds: ctx, min_ratio or max_ratio is NULL"; return CN_ERR_BAD_ARG; }
    *min_ratio = ctx->trust_min; *max_ratio = ctx->trust_max;
    return CN_OK;
}
int cn_layer_trust_ratio(cn_layer *layer, float *ratio, float *weight_norm, float *update_norm)
{
    if (!layer) { g_last_error = "cn_layer_trust_ratio: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        if (!layer->trainable) throw cn_error(CN_ERR_BAD_ARG, "cn_layer_trust_ratio: layer has no weights");
        LambRecord h{}; h.ratio = 1.0f;
        if (c->lamb_recs && layer->lamb_rec >= 0) {
            enter(c);
            HIP_CHECK(hipMemcpyAsync(&h, c->lamb_recs + layer->lamb_rec, sizeof(h), hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        if (ratio) *ratio = h.ratio;
        if (weight_norm) *weight_norm = h.nw;
        if (update_norm) *update_norm = h.nu;
    });
}

// ---------------------------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------------------------
int cn_ctx_timing_enable(cn_ctx *ctx, int enable)
{
    if (!ctx) { g_last_error = "cn_ctx_timing_enable: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] { enter(ctx); timing_collect(ctx); ctx->timing = enable != 0; });
}
int cn_ctx_timing_read(cn_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches)
{
    if (!ctx || kernel_class < 0 || kernel_class >= KC_COUNT) { g_last_error = "cn_ctx_timing_read: bad argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        timing_collect(ctx);
        if (total_ms) *total_ms = ctx->acc_ms[kernel_class];
        if (launches) *launches = ctx->acc_n[kernel_class];
    });
}
int cn_ctx_timing_reset(cn_ctx *ctx)
{
    if (!ctx) { g_last_error = "cn_ctx_timing_reset: ctx is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        timing_collect(ctx);
        for (int k = 0; k < KC_COUNT; ++k) { ctx->acc_ms[k] = 0; ctx->acc_n[k] = 0; }
    });
}

const char *cn_layer_recurrent_kernel(cn_layer *layer, int backward)
{
    // what the launchers instantiated on the layer's last forward / backward pass (empty before the first one)
    if (!layer || !layer->lstm) return "";
    return layer->kname[backward ? 1 : 0];
}

// ---------------------------------------------------------------------------------------------
// kernel-level test hooks (include/currennt_hip_debug.h)
// ---------------------------------------------------------------------------------------------
int cn_dbg_gemm_nt(cn_ctx *ctx, const float *A, const float *B, float *C, int M, int N, int K, const float *bias, int act)
{
    if (!ctx || !A || !B || !C) { g_last_error = "cn_dbg_gemm_nt: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (K % 8 || N % 32) throw cn_error(CN_ERR_SHAPE, "cn_dbg_gemm_nt: K must be a multiple of 8 and N of 32");
        const size_t e = ctx->esz();
        const Scratch sA((size_t)M * K * 4), sB((size_t)N * K * 4), sC((size_t)M * N * 4), sOA((size_t)M * K * e), sOB((size_t)N * K * e);
        Scratch sBias, sC2;
        float *dA = sA.get(), *dB = sB.get(), *dC = sC.get();
        void *oA = sOA.get<void>(), *oB = sOB.get<void>();
        HIP_CHECK(hipMemcpyAsync(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(dB, B, (size_t)N * K * 4, hipMemcpyHostToDevice, ctx->stream));
        if (bias) { sBias.alloc((size_t)N * 4); HIP_CHECK(hipMemcpyAsync(sBias.get(), bias, (size_t)N * 4, hipMemcpyHostToDevice, ctx->stream)); }
        float *dbias = sBias.get();
        launch_pad_convert(ctx->stream, ctx->f32, dA, M, K, oA, K);
        launch_pad_convert(ctx->stream, ctx->f32, dB, N, K, oB, K);
        // act | 0x100: both outputs (fp32 and operand-type copy), the COPY is returned; act | 0x200: the copy alone
        const bool both = act & 0x100, copy_only = act & 0x200;
        if (both || copy_only) sC2.alloc((size_t)M * N * e);
        void *dC2 = sC2.get<void>();
        GemmNT g{}; g.A = oA; g.lda = K; g.B = oB; g.ldb = K; g.C = copy_only ? nullptr : dC; g.ldc = N; g.C2 = dC2; g.ldc2 = N;
        g.bias = dbias; g.act = act & 0xff; g.M = M; g.N = N; g.K = K;
        launch_gemm_nt(ctx->stream, ctx->prec, g);
        HIP_CHECK(hipGetLastError());
        if (dC2 && e == 2) {
            std::vector<uint16_t> h((size_t)M * N);
            HIP_CHECK(hipMemcpyAsync(h.data(), dC2, h.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < h.size(); ++i) { const uint32_t u = (uint32_t)h[i] << 16; memcpy(&C[i], &u, 4); }
        } else {
            HIP_CHECK(hipMemcpyAsync(C, dC2 ? dC2 : dC, (size_t)M * N * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
    });
}

int cn_dbg_ctc(cn_ctx *ctx, const float *y, const char *pat, int T, int PS, int C, const int *labels, const int *label_lengths,
               float *loss_out, float *err_out)
{
    if (!ctx || !y || !pat || !label_lengths || !loss_out || !err_out) { g_last_error = "cn_dbg_ctc: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (T <= 0 || PS <= 0 || C < 2) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc: T, PS must be positive and C >= 2");
        int maxU = 0; size_t total = 0;
        for (int s = 0; s < PS; ++s) {
            if (label_lengths[s] < 0) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc: negative label sequence length");
            maxU = std::max(maxU, label_lengths[s]); total += (size_t)label_lengths[s];
        }
        if (total && !labels) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc: labels missing");
        for (size_t i = 0; i < total; ++i)
            if (labels[i] < 0 || labels[i] > C - 2) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc: label outside [0, C - 2]");
        const int PSp = round_up(PS, 4), Lp = round_up(C, 32), N = T * PSp;
        if (!ctc_shape_fits(maxU, Lp)) throw cn_error(CN_ERR_SHAPE, "cn_dbg_ctc: label sequences or rows too long for a workgroup");
        const size_t stride = std::max<size_t>(total, 1);
        std::vector<int> packed(3 * stride + PSp + 1, 0);
        const int maxS = ctc_pack_labels(packed.data(), labels, label_lengths, PS, PSp, stride, C);
        const int Sp = round_up(maxS, 64);
        // the caller's [T][PS] rows in the device's [T][PSp] pitch: pad slots are PATTYPE_NONE, pad columns zero
        std::vector<float> hy((size_t)N * Lp, 0.f); std::vector<char> hpat(N, 0);
        for (int t = 0; t < T; ++t)
            for (int s = 0; s < PS; ++s) {
                hpat[(size_t)t * PSp + s] = pat[(size_t)t * PS + s];
                memcpy(&hy[((size_t)t * PSp + s) * Lp], y + ((size_t)t * PS + s) * C, C * sizeof(float));
            }
        Scratch dy(hy.size() * sizeof(float)), dpat(N), dlab(packed.size() * sizeof(int)), dal((size_t)PSp * T * Sp * sizeof(int2)),
            dbe((size_t)PSp * T * Sp * sizeof(int2)), dinfo((size_t)PSp * 2 * sizeof(int)), drs((size_t)PSp * 2 * sizeof(float)), derr((size_t)N * Lp * sizeof(float));
        hipStream_t st = ctx->stream;
        HIP_CHECK(hipMemcpyAsync(dy.p, hy.data(), hy.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dpat.p, hpat.data(), N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dlab.p, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(drs.p, 0xFF, (size_t)PSp * 2 * sizeof(float), st));         // NaNs: the sweeps write every slot's pair
        HIP_CHECK(hipMemsetAsync(derr.p, 0xFF, (size_t)N * Lp * sizeof(float), st));        // NaNs: an element the launches leave out shows
        CtcArgs a{};
        a.y = dy.get(); a.pat = dpat.get<char>(); a.T = T; a.PSp = PSp; a.C = C; a.Lp = Lp;
        a.labels = dlab.get<int>(); a.next = a.labels + stride; a.first = a.next + stride; a.laboff = a.first + stride;
        a.maxS = maxS; a.alpha = dal.get<int2>(); a.beta = dbe.get<int2>(); a.Sp = Sp;
        a.info = dinfo.get<int>(); a.rowstat = drs.get(); a.err = derr.get();
        launch_ctc_sweeps(st, a);
        launch_ctc_errors(st, a);
        std::vector<float> hrs((size_t)PSp * 2), herr((size_t)N * Lp);
        HIP_CHECK(hipMemcpyAsync(hrs.data(), drs.p, hrs.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(herr.data(), derr.p, herr.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        // pad slots and pad columns are not part of the caller's layout: the hook itself holds them to the contract (exactly 0)
        for (int t = 0; t < T; ++t)
            for (int s = 0; s < PSp; ++s)
                for (int j = 0; j < Lp; ++j) {
                    const float v = herr[((size_t)t * PSp + s) * Lp + j];
                    if (s < PS && j < C) err_out[((size_t)t * PS + s) * C + j] = v;
                    else if (!(v == 0.f)) throw cn_error(CN_ERR_STATE, "cn_dbg_ctc: a pad slot or pad column of the output errors is not 0");
                }
        for (int s = 0; s < PS; ++s) loss_out[s] = hrs[2 * s];
    });
}

int cn_dbg_ctc_decode(cn_ctx *ctx, const float *y, const char *pat, int T, int PS, int C, const int *labels, const int *label_lengths,
                      int accumulate, int *argmax_out, int *decoded, int *decoded_lengths, int *distances)
{
    if (!ctx || !y || !pat) { g_last_error = "cn_dbg_ctc_decode: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (T <= 0 || PS <= 0 || C < 2) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc_decode: T, PS must be positive and C >= 2");
        if (accumulate && !label_lengths) throw cn_error(CN_ERR_STATE, "cn_dbg_ctc_decode: no label sequences to accumulate against");
        int maxU = 0; size_t total = 0;
        for (int s = 0; label_lengths && s < PS; ++s) {
            if (label_lengths[s] < 0) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc_decode: negative label sequence length");
            maxU = std::max(maxU, label_lengths[s]); total += (size_t)label_lengths[s];
        }
        if (total && !labels) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc_decode: labels missing");
        for (size_t i = 0; i < total; ++i)
            if (labels[i] < 0 || labels[i] > C - 2) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_ctc_decode: label outside [0, C - 2]");
        if (!ctc_decode_fits(T, maxU)) throw cn_error(CN_ERR_SHAPE, "cn_dbg_ctc_decode: min(T, longest label sequence) exceeds the distance's LDS bound");
        const int PSp = round_up(PS, 4), Lp = round_up(C, 32), N = T * PSp;
        const size_t stride = std::max<size_t>(total, 1);
        std::vector<int> packed(3 * stride + PSp + 1, 0);
        if (label_lengths) ctc_pack_labels(packed.data(), labels, label_lengths, PS, PSp, stride, C);
        // the caller's [T][PS] rows in the device's [T][PSp] pitch: pad slots are PATTYPE_NONE; pad columns hold +inf, which would win
        // every row if they took part
        std::vector<float> hy((size_t)N * Lp, INFINITY); std::vector<char> hpat(N, 0);
        for (int t = 0; t < T; ++t)
            for (int s = 0; s < PS; ++s) {
                hpat[(size_t)t * PSp + s] = pat[(size_t)t * PS + s];
                memcpy(&hy[((size_t)t * PSp + s) * Lp], y + ((size_t)t * PS + s) * C, C * sizeof(float));
            }
        const size_t ints = 2 * (size_t)N + 2 * (size_t)PSp;
        Scratch dy(hy.size() * sizeof(float)), dpat(N), dlab(packed.size() * sizeof(int)), dout(ints * sizeof(int));
        hipStream_t st = ctx->stream;
        HIP_CHECK(hipMemcpyAsync(dy.p, hy.data(), hy.size() * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dpat.p, hpat.data(), N, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dlab.p, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(dout.p, 0xFF, ints * sizeof(int), st));
        CtcDecodeArgs a{};
        a.pat = dpat.get<char>(); a.T = T; a.PSp = PSp; a.C = C;
        int *amax = dout.get<int>();
        a.amax = amax; a.decoded = amax + N; a.decoded_len = a.decoded + N; a.dist = a.decoded_len + PSp;
        if (label_lengths) { a.labels = dlab.get<int>(); a.laboff = a.labels + 3 * stride; }
        a.maxShort = std::min(T, maxU);
        a.sums = accumulate ? ctc_sums(ctx) : nullptr;
        launch_ctc_argmax(st, dy.get(), a.pat, N, C, Lp, amax);
        launch_ctc_collapse(st, a);
        std::vector<int> h(ints);
        HIP_CHECK(hipMemcpyAsync(h.data(), dout.p, ints * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        const int *hdec = h.data() + N, *hlen = hdec + N, *hdist = hlen + PSp;
        for (int s = PS; s < PSp; ++s)       // pad slots are not part of the caller's layout: the hook itself holds them to the contract
            if (hlen[s] != 0) throw cn_error(CN_ERR_STATE, "cn_dbg_ctc_decode: a pad slot decoded to something");
        for (int t = 0; t < T; ++t)
            for (int s = 0; s < PS; ++s)
                if (argmax_out) argmax_out[(size_t)t * PS + s] = h[(size_t)t * PSp + s];
        for (int s = 0; s < PS; ++s) {
            if (decoded) memcpy(decoded + (size_t)s * T, hdec + (size_t)s * T, (size_t)T * sizeof(int));
            if (decoded_lengths) decoded_lengths[s] = hlen[s];
            if (distances) distances[s] = hdist[s];
        }
    });
}

int cn_dbg_prefetch_hits(cn_ctx *ctx, int *hits)
{
    if (!ctx || !hits) { g_last_error = "cn_dbg_prefetch_hits: NULL argument"; return CN_ERR_BAD_ARG; }
    *hits = ctx->pf.hits;
    return CN_OK;
}

int cn_dbg_layer_axis(cn_layer *layer, char *pat, int *tcls, int *len, size_t rows, int *PSp)
{
    if (!layer) { g_last_error = "cn_dbg_layer_axis: layer is NULL"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        join_side(c);
        require_axis(layer, "cn_dbg_layer_axis");
        const TimeAxis *ax = layer->ax;
        if (PSp) *PSp = c->PSp;
        if ((pat || tcls) && rows != (size_t)ax->N) throw cn_error(CN_ERR_SHAPE, "cn_dbg_layer_axis: rows != T * padded parallel sequences");
        // (refused BEFORE the length pass: without a context layer the table it would write does not exist)
        if (len && !ax->len) throw cn_error(CN_ERR_STATE, "cn_dbg_layer_axis: the context has no context layer, so no slot lengths");
        if (len && !ax->owner) context_lengths(c);
        if (pat) HIP_CHECK(hipMemcpyAsync(pat, ax->pat, rows, hipMemcpyDeviceToHost, c->stream));
        if (tcls) HIP_CHECK(hipMemcpyAsync(tcls, ax->tcls, rows * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (len) HIP_CHECK(hipMemcpyAsync(len, ax->len, (size_t)c->PSp * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    });
}

int cn_dbg_layer_pad_bits(cn_layer *layer, long long *nonzero)
{
    if (!layer || !nonzero) { g_last_error = "cn_dbg_layer_pad_bits: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        cn_ctx *c = layer->ctx;
        enter(c);
        require_loaded(c);
        join_side(c);
        require_axis(layer, "cn_dbg_layer_pad_bits");
        if (!layer->out_op) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_layer_pad_bits: layer has no outputs");
        const UnitMap m = unit_map(layer);
        const size_t rows = (size_t)layer->ax->N, e = c->esz();
        std::vector<unsigned char> h(rows * m.Lp * e);
        HIP_CHECK(hipMemcpyAsync(h.data(), follower_operand(layer), h.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        long long n = 0;
        for (size_t r = 0; r < rows; ++r) {
            const bool pad_slot = (int)(r % c->PSp) >= c->PS;
            for (int col = 0; col < m.Lp; ++col) {
                if (!pad_slot && m.unit(col) >= 0) continue;
                bool any = false;
                for (size_t b = 0; b < e; ++b) any = any || h[(r * m.Lp + col) * e + b] != 0;
                n += any;
            }
        }
        *nonzero = n;
    });
}

int cn_dbg_row_map_counts(cn_ctx *ctx, int out[3])
{
    if (!ctx || !out) { g_last_error = "cn_dbg_row_map_counts: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        require_loaded(ctx);
        join_side(ctx);
        HIP_CHECK(hipMemcpyAsync(out, ctx->rowmap_of(ctx->d_pat_raw), 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        out[2] = ctx->N;
    });
}

int cn_dbg_gemm_tn(cn_ctx *ctx, const float *A, const float *B, float *C, int M, int N, int K)
{
    if (!ctx || !A || !B || !C) { g_last_error = "cn_dbg_gemm_tn: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (M % 32 || N % 32) throw cn_error(CN_ERR_SHAPE, "cn_dbg_gemm_tn: M and N must be multiples of 32");
        const size_t e = ctx->esz();
        const Scratch sA((size_t)M * K * 4), sB((size_t)N * K * 4), sC((size_t)M * N * 4), sOA((size_t)M * K * e), sOB((size_t)N * K * e);
        float *dA = sA.get(), *dB = sB.get(), *dC = sC.get();
        void *oA = sOA.get<void>(), *oB = sOB.get<void>();
        HIP_CHECK(hipMemcpyAsync(dA, A, (size_t)M * K * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(dB, B, (size_t)N * K * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemsetAsync(dC, 0, (size_t)M * N * 4, ctx->stream));
        launch_pad_convert(ctx->stream, ctx->f32, dA, K, M, oA, M);
        launch_pad_convert(ctx->stream, ctx->f32, dB, K, N, oB, N);
        GemmTN g{}; g.A = oA; g.lda = M; g.B = oB; g.ldb = N; g.C = dC; g.ldc = N; g.M = M; g.N = N; g.K = K;
        launch_gemm_tn(ctx->stream, ctx->prec, g);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"

namespace {

static_assert(CN_DBG_MAX_SPLITS == DET_MAX_SPLITS, "currennt_hip_debug.h states the workspace depth of cn_internal.h");

// a host fold item of the test hooks on the device: checked, uploaded, and read back behind the launch
struct DbgFold {
    std::deque<Scratch> mem;
    FoldItem f{};
    const cn_dbg_fold_item *h = nullptr;
    size_t dst_n = 0, part_n = 0;
    static void validate(const cn_dbg_fold_item &h, const char *who)
    {
        const std::string w(who);
        if (h.nparts < 1 || h.rows < 0 || h.cols < 0 || h.ld < 0) throw cn_error(CN_ERR_BAD_ARG, w + ": fold item with nparts < 1 or a negative size");
        if (h.cols > h.ld) throw cn_error(CN_ERR_SHAPE, w + ": fold item with cols > ld");
        if (h.rows && h.cols && h.stride < (long long)(h.rows - 1) * h.ld + h.cols) throw cn_error(CN_ERR_SHAPE, w + ": fold item whose partials overlap (stride)");
        if (h.rows && h.cols && (!h.dst || !h.part)) throw cn_error(CN_ERR_BAD_ARG, w + ": fold item with a NULL dst or part");
    }
    void upload(cn_ctx *ctx, const cn_dbg_fold_item &item)
    {
        h = &item;
        dst_n = (size_t)item.rows * item.ld;
        part_n = (item.rows && item.cols) ? (size_t)item.nparts * (size_t)item.stride : 0;
        float *dst = (float *)mem.emplace_back(std::max<size_t>(dst_n * 4, 16)).get();
        float *part = (float *)mem.emplace_back(std::max<size_t>(part_n * 4, 16)).get();
        if (dst_n) HIP_CHECK(hipMemcpyAsync(dst, item.dst, dst_n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (part_n) HIP_CHECK(hipMemcpyAsync(part, item.part, part_n * 4, hipMemcpyHostToDevice, ctx->stream));
        f = FoldItem{dst, part, (long)item.stride, item.nparts, item.rows, item.cols, item.ld, item.accumulate, item.clear};
    }
    void download(cn_ctx *ctx) const
    {
        if (dst_n) HIP_CHECK(hipMemcpyAsync(h->dst, f.dst, dst_n * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (part_n && h->clear) HIP_CHECK(hipMemcpyAsync(h->part, f.part, part_n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
};

}  // namespace

extern "C" {

int cn_dbg_gemm_tn_group(cn_ctx *ctx, const cn_dbg_tn_item *items, int n, int cu_budget, int flags, int *splits_out,
                         const cn_dbg_fold_item *extra)
{
    if (!ctx || (n > 0 && !items)) { g_last_error = "cn_dbg_gemm_tn_group: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        const char *who = "cn_dbg_gemm_tn_group";
        const std::string w(who);
        const bool defer = flags & 1;
        const int e = (int)ctx->esz(), al = 16 / e;
        if (n < 0 || n > 3) throw cn_error(CN_ERR_BAD_ARG, w + ": 0 to 3 items");
        if (cu_budget < 0 || (flags & ~1)) throw cn_error(CN_ERR_BAD_ARG, w + ": negative cu_budget or unknown flag");
        if (defer && !ctx->det) throw cn_error(CN_ERR_BAD_ARG, w + ": the deferred form needs the deterministic option");
        if (defer && !splits_out) throw cn_error(CN_ERR_BAD_ARG, w + ": the deferred form needs splits_out");
        auto live = [](const cn_dbg_tn_item &it) { return it.M > 0 && it.N > 0 && it.K > 0; };
        for (int i = 0; i < n; ++i) {
            const cn_dbg_tn_item &it = items[i];
            if (it.M < 0 || it.N < 0 || it.K < 0) throw cn_error(CN_ERR_BAD_ARG, w + ": negative M, N or K");
            if (it.M % 32 || it.N % 32) throw cn_error(CN_ERR_SHAPE, w + ": M and N must be multiples of 32");
            if (!live(it)) continue;
            if (!it.A || !it.B || !it.C) throw cn_error(CN_ERR_BAD_ARG, w + ": NULL A, B or C");
            if (it.ldc < it.N) throw cn_error(CN_ERR_SHAPE, w + ": ldc < N");
            if (it.a_row < 0 || it.a_col < 0 || it.b_row < 0 || it.b_col < 0 || it.rows_a < 0 || it.rows_b < 0 ||
                (long)it.a_row + it.K > it.rows_a || (long)it.a_col + it.M > it.lda ||
                (long)it.b_row + it.K > it.rows_b || (long)it.b_col + it.N > it.ldb)
                throw cn_error(CN_ERR_SHAPE, w + ": a view leaves its parent");
            if (it.lda % al || it.ldb % al || it.a_col % al || it.b_col % al)
                throw cn_error(CN_ERR_SHAPE, w + ": pitches and column offsets must keep the views 16-byte aligned in the operand type");
        }
        if (extra) DbgFold::validate(*extra, who);

        // one device copy per distinct host parent, converted whole
        std::deque<Scratch> mem;
        struct Parent { const float *host; int rows, ld; char *op; };
        std::vector<Parent> parents;
        auto parent = [&](const float *host, int rows, int ld) -> char * {
            for (const Parent &p : parents) if (p.host == host && p.rows == rows && p.ld == ld) return p.op;
            const size_t count = (size_t)rows * ld;
            const Scratch stage(count * 4);
            char *op = mem.emplace_back(count * e).get<char>();
            HIP_CHECK(hipMemcpyAsync(stage.get(), host, count * 4, hipMemcpyHostToDevice, ctx->stream));
            launch_pad_convert(ctx->stream, ctx->f32, stage.get(), rows, ld, op, ld);
            HIP_CHECK(hipStreamSynchronize(ctx->stream));        // (the staging copy goes with this scope)
            parents.push_back(Parent{host, rows, ld, op});
            return op;
        };
        GemmTN gs[3]; int used[3] = {0, 0, 0};
        float *dC[3] = {nullptr, nullptr, nullptr}, *dWs[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < n; ++i) {
            const cn_dbg_tn_item &it = items[i];
            GemmTN g{};
            g.M = it.M; g.N = it.N; g.K = it.K; g.lda = it.lda; g.ldb = it.ldb; g.ldc = it.ldc;
            if (live(it)) {
                g.A = parent(it.A, it.rows_a, it.lda) + ((size_t)it.a_row * it.lda + it.a_col) * e;
                g.B = parent(it.B, it.rows_b, it.ldb) + ((size_t)it.b_row * it.ldb + it.b_col) * e;
                const size_t cn = (size_t)it.M * it.ldc;
                dC[i] = mem.emplace_back(cn * 4).get();
                if (!defer) HIP_CHECK(hipMemcpyAsync(dC[i], it.C, cn * 4, hipMemcpyHostToDevice, ctx->stream));
                g.C = dC[i];
                if (ctx->det) {
                    dWs[i] = mem.emplace_back((size_t)DET_MAX_SPLITS * cn * 4).get();
                    const float sentinel = CN_DBG_WS_SENTINEL; int bits; memcpy(&bits, &sentinel, 4);
                    HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)dWs[i], bits, (size_t)DET_MAX_SPLITS * cn, ctx->stream));
                    g.ws = dWs[i]; g.ws_splits = DET_MAX_SPLITS; g.ws_used = defer ? &used[i] : nullptr;
                }
            }
            gs[i] = g;
        }
        DbgFold xf;
        if (extra) xf.upload(ctx, *extra);
        launch_gemm_tn_group(ctx->stream, ctx->prec, gs, n, cu_budget, extra ? &xf.f : nullptr);
        HIP_CHECK(hipGetLastError());
        for (int i = 0; i < n; ++i) {
            if (splits_out) splits_out[i] = used[i];
            if (!dC[i]) continue;
            const size_t cn = (size_t)items[i].M * items[i].ldc;
            if (defer) HIP_CHECK(hipMemcpyAsync(items[i].C, dWs[i], (size_t)DET_MAX_SPLITS * cn * 4, hipMemcpyDeviceToHost, ctx->stream));
            else HIP_CHECK(hipMemcpyAsync(items[i].C, dC[i], cn * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (extra) xf.download(ctx);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int cn_dbg_fold(cn_ctx *ctx, const cn_dbg_fold_item *items, int n)
{
    if (!ctx || (n > 0 && !items)) { g_last_error = "cn_dbg_fold: NULL argument"; return CN_ERR_BAD_ARG; }
    return guarded([&] {
        enter(ctx);
        if (n < 0) throw cn_error(CN_ERR_BAD_ARG, "cn_dbg_fold: negative item count");
        for (int i = 0; i < n; ++i) DbgFold::validate(items[i], "cn_dbg_fold");
        std::deque<DbgFold> dev;
        std::vector<FoldItem> fs;
        for (int i = 0; i < n; ++i) { dev.emplace_back().upload(ctx, items[i]); fs.push_back(dev.back().f); }
        launch_fold(ctx->stream, fs.data(), n);
        HIP_CHECK(hipGetLastError());
        for (const DbgFold &d : dev) d.download(ctx);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
