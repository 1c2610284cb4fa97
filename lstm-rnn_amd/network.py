"""Host-side mirror of NeuralNetwork<TDevice> / Layer<TDevice> over the C ABI.

Method names and call order follow currennt_lib/src/NeuralNetwork.cpp:37-130 (construction from
the "layers"/"weights" JSON sections), :161-190 (loadSequences / computeForwardPass /
computeBackwardPass / calculateError), :237-262 (getOutputs) and
optimizers/SteepestDescentOptimizer.cu:67-94 (_updateWeights).  All arithmetic happens in
libcurrennt_hip.so; nothing here touches the CPU oracle.
"""
import ctypes as C

import numpy as np

from . import binding as B

_TRAINABLE = ("lstm", "blstm", "softmax", "feedforward_tanh", "feedforward_logistic",
              "feedforward_identity")
_RESIDUAL = ("lstm", "blstm", "feedforward_tanh", "feedforward_logistic", "feedforward_identity")
_POST = ("sse", "multiclass_classification", "weightedsse", "wf", "ce", "rmse", "binary_classification", "ctc")


class Layer:
    """One layer handle (layers/Layer.hpp:40-179, TrainableLayer.hpp:84-155)."""

    def __init__(self, net, desc, prev):
        self.net, self.desc, self.prev = net, desc, prev
        if "name" not in desc:
            raise RuntimeError("Missing value 'name' in layer description")           # Layer.cpp:52-53
        if "size" not in desc:
            raise RuntimeError("Missing value 'size' in layer '%s'" % desc["name"])   # Layer.cpp:56-57
        self.name, self.type, self.size = desc["name"], desc["type"], int(desc["size"])
        if self.type not in B.LAYER_KINDS and self.type != "context":
            raise RuntimeError("Unknown layer type '%s'" % self.type)                  # LayerFactory.cu:86
        self.trainable = self.type in _TRAINABLE
        self.post = self.type in _POST
        if self.trainable and "bias" not in desc:
            raise RuntimeError("Missing value 'bias' in layer '%s'" % self.name)       # TrainableLayer.cu:61-62
        self.bias = float(desc.get("bias", 0.0))
        self.learning_rate = float(desc.get("learningRate", -1.0))                     # TrainableLayer.cu:58
        if prev is not None and self.post and getattr(prev, "residual", False):       # (as the C++ driver; the library refuses the layer too)
            raise RuntimeError("Invalid value 'residual' in layer '%s': a post output layer cannot follow a residual layer directly" % prev.name)
        h = C.c_void_p()
        L = net.lib
        if self.type == "context":
            # "left" / "right" (default 0) neighbouring frames of the preceding layer at steps of "dilation" (default 1) beside
            # each frame (include/currennt_hip.h, section Context layers).  The size is checked here, with the reference's text;
            # the members' ranges are the library's to refuse (CN_ERR_BAD_ARG)
            if prev is None:
                raise RuntimeError("The first layer is not an input layer")
            self.left, self.right, self.dilation = self._int_member(desc, "left", 0), self._int_member(desc, "right", 0), self._int_member(desc, "dilation", 1)
            # "stride" (default 1): the layer keeps every stride-th frame and starts a new time axis (section Strided context layers)
            self.stride_member = self._int_member(desc, "stride", 1)
            blocks = self.left + self.right + 1
            if blocks >= 1 and self.size != blocks * prev.size:
                raise RuntimeError("Size mismatch: %d vs. %d in layer '%s' (%d frames of the preceding layer's %d units)"
                                   % (self.size, blocks * prev.size, self.name, blocks, prev.size))
            if "stride" in desc:
                B.check(L.cn_layer_create_context_strided(net.ctx, prev.handle, self.left, self.right, self.dilation, self.stride_member,
                                                          C.byref(h)), net.ctx)
            else:
                B.check(L.cn_layer_create_context(net.ctx, prev.handle, self.left, self.right, self.dilation, C.byref(h)), net.ctx)
        else:
            B.check(L.cn_layer_create(net.ctx, B.LAYER_KINDS[self.type], prev.handle if prev else None,
                                      self.size, self.bias,
                                      net.parallel_sequences if prev is None else 0,
                                      net.max_seq_length if prev is None else 0, C.byref(h)), net.ctx)
        self.handle = h
        # the product of the strides in front of (and of) this layer: its read-backs are sized by ceil(T / rate)
        self.rate = (prev.rate if prev is not None else 1) * (self.stride_member if self.type == "context" else 1)
        self.weight_count = L.cn_layer_weight_count(h) if self.trainable else 0
        if self.trainable and self.learning_rate >= 0.0:       # cn_sgd_update_all honours it too (SteepestDescentOptimizer.cu:78-80)
            B.check(L.cn_layer_set_learning_rate(h, self.learning_rate), net.ctx)
        # "dropout": rate of the dropout on this layer's input (include/currennt_hip.h, section Dropout); absent = none
        self.dropout = float(desc.get("dropout", 0.0))
        if "dropout" in desc:
            # (the same two refusals, with the same texts, as the C++ driver's Layer / TrainableLayer constructors)
            if not self.trainable:
                raise RuntimeError("Invalid value 'dropout' in layer '%s': only lstm, blstm, feedforward_* and softmax layers take dropout" % self.name)
            if not 0.0 <= self.dropout < 1.0:
                raise RuntimeError("Invalid value 'dropout' in layer '%s': the rate must lie in [0, 1)" % self.name)
            self.set_dropout(self.dropout)
        # "residual": followers read this layer's output plus its input (include/currennt_hip.h, section Residual connections)
        self.residual = False
        if "residual" in desc:
            # (the same refusals, with the same texts, as the C++ driver's Layer constructor)
            if not isinstance(desc["residual"], bool):
                raise RuntimeError("Invalid value 'residual' in layer '%s': true or false expected" % self.name)
            if self.type not in _RESIDUAL:
                raise RuntimeError("Invalid value 'residual' in layer '%s': only lstm, blstm and feedforward_* layers can be residual" % self.name)
            if desc["residual"]:
                if self.size != prev.size:
                    raise RuntimeError("Invalid value 'residual' in layer '%s': the layer's size %d differs from the preceding layer's size %d"
                                       % (self.name, self.size, prev.size))
                self.set_residual(True)
        # "layer_norm": this layer's input products read a normalised copy of its input (include/currennt_hip.h, section Layer
        # normalization); "layer_norm_eps": the eps under the square root, default 1e-5
        self.layer_norm, self.layer_norm_eps = False, 1e-5
        if "layer_norm" in desc or "layer_norm_eps" in desc:
            # (the same refusals, with the same texts, as the C++ driver's Layer constructor)
            member = "layer_norm" if "layer_norm" in desc else "layer_norm_eps"
            if not self.trainable:
                raise RuntimeError("Invalid value '%s' in layer '%s': only lstm, blstm, feedforward_* and softmax layers normalise their input"
                                   % (member, self.name))
            if not isinstance(desc.get("layer_norm", False), bool):
                raise RuntimeError("Invalid value 'layer_norm' in layer '%s': true or false expected" % self.name)
            eps = desc.get("layer_norm_eps", 1e-5)
            if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not (0.0 < float(eps) < float("inf")):
                raise RuntimeError("Invalid value 'layer_norm_eps' in layer '%s': a finite number above 0 expected" % self.name)
            self.layer_norm_eps = float(eps)
            if desc.get("layer_norm", False):
                if prev.size < 2:
                    raise RuntimeError("Invalid value 'layer_norm' in layer '%s': the preceding layer's size %d is below 2" % (self.name, prev.size))
                self.set_layer_norm(True, self.layer_norm_eps)
        if self.type in ("lstm", "blstm"):
            self.dirs = 2 if self.type == "blstm" else 1
            self.H = self.size // self.dirs

    def _int_member(self, desc, member, default):
        v = desc.get(member, default)
        if isinstance(v, bool) or not isinstance(v, int):
            raise RuntimeError("Invalid value '%s' in layer '%s': an integer expected" % (member, self.name))
        return v

    def context(self):
        """cn_layer_context: (left, right, dilation) of a context layer."""
        l, r, d = C.c_int(), C.c_int(), C.c_int()
        B.check(self.net.lib.cn_layer_context(self.handle, C.byref(l), C.byref(r), C.byref(d)), self.net.ctx)
        return l.value, r.value, d.value

    def stride(self):
        """cn_layer_context_stride: the stride of a context layer (1: a plain one)."""
        s = C.c_int()
        B.check(self.net.lib.cn_layer_context_stride(self.handle, C.byref(s)), self.net.ctx)
        return s.value

    def time(self):
        """cn_layer_time: (T, Tmin, rate) -- the steps of the current fraction as this layer sees them and the product of the
        strides in front of it."""
        t, tmin, r = C.c_int(), C.c_int(), C.c_int()
        B.check(self.net.lib.cn_layer_time(self.handle, C.byref(t), C.byref(tmin), C.byref(r)), self.net.ctx)
        return t.value, tmin.value, r.value

    @property
    def T(self):
        """Time steps of the fraction loaded last in this layer's own time axis."""
        return -(-self.net.T // self.rate)

    @property
    def N(self):
        return self.T * self.net.PS

    def pad_bits(self):
        """cn_dbg_layer_pad_bits: elements with a non-zero bit in the pad columns and pad slots of the rows this layer's followers
        read (what outputs() cannot show)."""
        n = C.c_longlong(-1)
        B.check(self.net.lib.cn_dbg_layer_pad_bits(self.handle, C.byref(n)), self.net.ctx)
        return n.value

    def forward(self):
        """cn_layer_forward of this layer alone."""
        B.check(self.net.lib.cn_layer_forward(self.handle), self.net.ctx)

    def backward(self):
        """cn_layer_backward of this layer alone."""
        B.check(self.net.lib.cn_layer_backward(self.handle), self.net.ctx)

    # -- buffers in reference layout -----------------------------------------------------------
    def _read(self, which, count, direction=0):
        out = np.empty(count, np.float32)
        B.check(self.net.lib.cn_layer_read(self.handle, B.BUF[which], direction,
                                           out.ctypes.data_as(C.c_void_p), count), self.net.ctx)
        return out

    def outputs(self):
        return self._read("outputs", self.N * self.size).reshape(self.T, self.net.PS, self.size)

    def output_errors(self):
        return self._read("outputErrors", self.N * self.size).reshape(self.T, self.net.PS, self.size)

    def weights(self):
        return self._read("weights", self.weight_count)

    def weight_updates(self):
        return self._read("weightUpdates", self.weight_count)

    def first_moments(self):
        """Adam's first moments m: the weightDeltas vector of a context that updates with Adam."""
        return self._read("weightDeltas", self.weight_count)

    def second_moments(self):
        """Adam's second moments v (zeros before the context's first Adam call)."""
        return self._read("adamSecondMoments", self.weight_count)

    def trust_ratio(self):
        """cn_layer_trust_ratio: (ratio, weight_norm, update_norm) of the layer's last LAMB step as np.float32; (1, 0, 0) before
        the first."""
        f = [C.c_float() for _ in range(3)]
        B.check(self.net.lib.cn_layer_trust_ratio(self.handle, C.byref(f[0]), C.byref(f[1]), C.byref(f[2])), self.net.ctx)
        return tuple(np.float32(x.value) for x in f)

    def upload(self, which, array):
        """cn_layer_upload: overwrite a flat parameter vector ("weights", "weightUpdates", "weightDeltas",
        "adamSecondMoments") from the host."""
        flat = np.ascontiguousarray(array, np.float32).reshape(-1)
        B.check(self.net.lib.cn_layer_upload(self.handle, B.BUF[which], flat.ctypes.data_as(C.c_void_p), flat.size),
                self.net.ctx)

    def weight_average(self):
        """cn_layer_read_weight_average: this layer's part of the context's weight average (include/currennt_hip.h, section Weight
        averaging); before an average exists: the weights.  While swapped it holds the raw weights."""
        out = np.empty(self.weight_count, np.float32)
        B.check(self.net.lib.cn_layer_read_weight_average(self.handle, out.ctypes.data_as(C.c_void_p), out.size), self.net.ctx)
        return out

    def upload_weight_average(self, array):
        """cn_layer_upload_weight_average: overwrite this layer's part of the average from the host (autosave); creates the average
        as a copy of all weights if there is none."""
        flat = np.ascontiguousarray(array, np.float32).reshape(-1)
        B.check(self.net.lib.cn_layer_upload_weight_average(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size), self.net.ctx)

    def set_dropout(self, rate):
        """cn_layer_set_dropout: the rate of the dropout on this layer's input (0: none)."""
        B.check(self.net.lib.cn_layer_set_dropout(self.handle, float(rate)), self.net.ctx)
        self.dropout = float(rate)

    def dropout_input(self):
        """The masked operand copy this layer's input products read in its last forward pass, [T][PS][size of the preceding
        layer] (cn_dbg_dropout_input); CN_ERR_STATE when that pass did not drop."""
        n = self.N * self.prev.size
        out = np.empty(n, np.float32)
        B.check(self.net.lib.cn_dbg_dropout_input(self.handle, out.ctypes.data_as(C.c_void_p), n), self.net.ctx)
        return out.reshape(self.T, self.net.PS, self.prev.size)

    def set_residual(self, enable=True):
        """cn_layer_set_residual: from this layer's next forward pass on, its followers and outputs() see its own output plus
        what its preceding layer's followers see."""
        B.check(self.net.lib.cn_layer_set_residual(self.handle, 1 if enable else 0), self.net.ctx)
        self.residual = bool(enable)

    def residual_branch(self):
        """This layer's own output in its last forward pass, [T][PS][size] (cn_dbg_residual_branch): outputs() minus the skip
        path; CN_ERR_STATE when that pass did not sum."""
        n = self.N * self.size
        out = np.empty(n, np.float32)
        B.check(self.net.lib.cn_dbg_residual_branch(self.handle, out.ctypes.data_as(C.c_void_p), n), self.net.ctx)
        return out.reshape(self.T, self.net.PS, self.size)

    def set_layer_norm(self, enable=True, eps=1e-5):
        """cn_layer_set_layer_norm: from this layer's next forward pass on, its input products read the normalised copy of what
        its preceding layer's followers see (no gain, no bias: the input and bias weights absorb them)."""
        B.check(self.net.lib.cn_layer_set_layer_norm(self.handle, 1 if enable else 0, float(eps)), self.net.ctx)
        self.layer_norm, self.layer_norm_eps = bool(enable), float(eps)

    def normalized_input(self):
        """The normalised copy of this layer's input in its last forward pass, [T][PS][size of the preceding layer]
        (cn_dbg_layer_norm_input); CN_ERR_STATE when that pass did not normalise."""
        n = self.N * self.prev.size
        out = np.empty(n, np.float32)
        B.check(self.net.lib.cn_dbg_layer_norm_input(self.handle, out.ctypes.data_as(C.c_void_p), n), self.net.ctx)
        return out.reshape(self.T, self.net.PS, self.prev.size)

    def noisy_weights(self):
        """The weights this layer's last backward pass read, flat reference layout (cn_dbg_noisy_weights): w + noise as the noisy
        operand copies hold it, the bias entries clean; CN_ERR_STATE when that pass had no weight noise."""
        out = np.empty(self.weight_count, np.float32)
        B.check(self.net.lib.cn_dbg_noisy_weights(self.handle, out.ctypes.data_as(C.c_void_p), self.weight_count), self.net.ctx)
        return out

    def weight_updates_tensor(self, torch):
        """The layer's weightUpdates in HBM as a torch tensor aliasing the library's memory (no copy)."""
        if getattr(self, "_wu_tensor", None) is None:
            from .parallel import DeviceArray
            ptr = self.net.lib.cn_layer_device_ptr(self.handle, B.BUF["weightUpdates"])
            if not ptr:
                raise RuntimeError("layer '%s' has no weightUpdates in device memory" % self.name)
            self._wu_tensor = torch.as_tensor(DeviceArray(ptr, self.weight_count), device="cuda:%d" % self.net.device)
        return self._wu_tensor

    def internal(self, which, direction=0):
        """LSTM per-direction internal vector by its reference name (LstmLayer.hpp:88-100)."""
        return self._read(which, self.N * self.H, direction).reshape(self.T, self.net.PS, self.H)

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        B.check(self.net.lib.cn_layer_set_weights(self.handle, flat.ctypes.data_as(C.c_void_p), flat.size),
                self.net.ctx)

    def write_output_errors(self, err):
        err = np.ascontiguousarray(err, np.float32).reshape(-1)
        B.check(self.net.lib.cn_layer_write_output_errors(self.handle, err.ctypes.data_as(C.c_void_p), err.size),
                self.net.ctx)


class NeuralNetwork:
    def __init__(self, layers, weights=None, parallel_sequences=1, max_seq_length=1,
                 precision=B.PREC_F32, device=0, stream=None, seed=None, deterministic=None, options=None):
        self.lib = B.load_library()
        self.parallel_sequences, self.max_seq_length = int(parallel_sequences), int(max_seq_length)
        self.PS = self.parallel_sequences
        self.precision = precision
        self.device = int(device)
        ctx = C.c_void_p()
        B.check(self.lib.cn_ctx_create(device, precision, stream, C.byref(ctx)))
        self.ctx = ctx
        if deterministic is not None:                 # None: the library's default (on in the parity modes, off for bf16)
            self.set_option("deterministic", 1 if deterministic else 0)
        for name, value in (options or {}).items():   # options that size allocations ("ctc_max_labels") belong before the layers
            self.set_option(name, value)
        self.layers = []
        self.T = self.Tmin = self.N = 0
        self._lens = self._lens_from = None
        self.frame_skip = 1                               # set_input_splice: loads take source-rate fractions, read-backs go by ceil(T / k)
        try:
            names = set()
            prev = None
            for desc in layers:                                                        # NeuralNetwork.cpp:60-95
                lay = Layer(self, desc, prev)
                if lay.name in names:
                    raise RuntimeError("Different layers have the same name '%s'" % lay.name)   # :85-86
                names.add(lay.name)
                self.layers.append(lay)
                prev = lay
            if len(self.layers) < 3:
                raise RuntimeError("Not enough layers defined")                        # :98-99
            if self.layers[0].type != "input":
                raise RuntimeError("The first layer is not an input layer")            # :102-105 (paraphrased)
            if not self.layers[-1].post:
                raise RuntimeError("The last layer is not a post output layer")        # :116-117
            rng = np.random.RandomState(seed) if seed is not None else None
            for lay in self.layers:
                if not lay.trainable:
                    continue
                if weights is not None and lay.name in weights:                        # TrainableLayer.cu:68-101
                    w = weights[lay.name]
                    for key in ("input", "bias", "internal"):
                        if key not in w:
                            raise RuntimeError("Missing array 'weights/%s/%s'" % (lay.name, key))
                    flat = np.concatenate([np.asarray(w["input"], np.float32).reshape(-1),
                                           np.asarray(w["bias"], np.float32).reshape(-1),
                                           np.asarray(w["internal"], np.float32).reshape(-1)])
                    if flat.size != lay.weight_count:
                        raise RuntimeError("Invalid number of weights for layer '%s'" % lay.name)
                elif rng is not None:
                    # uniform [-0.1, 0.1] like Configuration.cpp:186-187; the reference draws from
                    # boost::mt19937, which is not reproducible here
                    flat = rng.uniform(-0.1, 0.1, lay.weight_count).astype(np.float32)
                else:
                    raise RuntimeError("no weights given for layer '%s' and no seed" % lay.name)
                lay.set_weights(flat)
        except Exception:
            self.close()
            raise

    # -- life cycle ----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.cn_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- NeuralNetwork API ---------------------------------------------------------------------
    def input_layer(self):
        return self.layers[0]

    def post_output_layer(self):
        return self.layers[-1]

    def output_layer(self):
        return self.layers[-2]

    def trainable_layers(self):
        return [l for l in self.layers if l.trainable]

    def layer(self, name):
        for l in self.layers:
            if l.name == name:
                return l
        raise KeyError(name)

    def _host_descriptor(self, frac):
        x = np.ascontiguousarray(frac["inputs"], np.float32)
        pat = np.ascontiguousarray(frac["patTypes"], np.int8)
        f = B.Fraction()
        f.max_seq_length, f.min_seq_length = int(frac["T"]), int(frac["Tmin"])
        f.num_sequences = int(frac.get("numSeqs", self.PS))
        f.input_pattern_size = int(x.shape[-1])
        keep = [x, pat]
        f.pat_types = pat.ctypes.data_as(C.c_void_p)
        f.inputs = x.ctypes.data_as(C.c_void_p)
        post = self.layers[-1]
        if "targetClasses" in frac and frac["targetClasses"] is not None:
            tc = np.ascontiguousarray(frac["targetClasses"], np.int32)
            keep.append(tc)
            f.target_classes = tc.ctypes.data_as(C.c_void_p)
            f.output_pattern_size = int(frac.get("outputPatternSize", post.size))
        if "targets" in frac and frac["targets"] is not None:
            tg = np.ascontiguousarray(frac["targets"], np.float32)
            keep.append(tg)
            f.targets = tg.ctypes.data_as(C.c_void_p)
            f.output_pattern_size = int(tg.shape[-1])
        return f, keep

    def load_sequences(self, frac):                                                    # NeuralNetwork.cpp:161-166
        f, keep = self._host_descriptor(frac)
        # (the library copies the host arrays into pinned staging memory before it returns: nothing to wait for)
        B.check(self.lib.cn_fraction_load(self.ctx, self.layers[0].handle, self.layers[-1].handle, C.byref(f)), self.ctx)
        self._set_current(f, (frac["patTypes"], int(frac["T"]), self.frame_skip))
        if self.layers[-1].type == "ctc" and frac.get("labels") is not None:
            self.set_label_sequences(frac["labels"])

    def _set_current(self, f, lens=None):
        """The lengths of the fraction just loaded as the layers see them: f's, or ceil(f's / frame_skip) under set_input_splice."""
        k = self.frame_skip
        self.T, self.Tmin = -(-f.max_seq_length // k), -(-f.min_seq_length // k)
        self.N = self.T * self.PS
        self._num_seqs = int(f.num_sequences)
        # lengths(): counted on demand, from the host's pattern types (kept by reference with their T) or, after a resident load,
        # from the device's
        self._lens, self._lens_from = None, lens

    def set_label_sequences(self, labels):
        """cn_layer_set_label_sequences: one int array of labels per sequence of the fraction loaded last (a ctc net)."""
        lens = np.asarray([len(l) for l in labels], np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).reshape(-1) for l in labels] + [np.zeros(0, np.int32)]))
        B.check(self.lib.cn_layer_set_label_sequences(self.layers[-1].handle, flat.ctypes.data_as(C.c_void_p),
                                                      lens.ctypes.data_as(C.c_void_p), len(labels)), self.ctx)

    def prefetch_sequences(self, frac):
        """cn_fraction_prefetch: `frac` (host arrays, as for load_sequences) is what the next load_sequences will load -- the
        reference's loader thread one fraction ahead (DataSet.cpp:202-240), here across PCIe and through the re-layout as well.
        The arrays must be the same objects (already contiguous float32 / int8 / int32) at that load: it matches by address."""
        f, keep = self._host_descriptor(frac)
        B.check(self.lib.cn_fraction_prefetch(self.ctx, self.layers[0].handle, self.layers[-1].handle, C.byref(f)), self.ctx)

    def _resident_descriptor(self, dfrac):
        f = B.Fraction()
        f.max_seq_length, f.min_seq_length = int(dfrac["T"]), int(dfrac["Tmin"])
        f.num_sequences = int(dfrac.get("numSeqs", self.PS))
        f.input_pattern_size = int(dfrac["inputPatternSize"])
        f.output_pattern_size = int(dfrac.get("outputPatternSize", self.layers[-1].size))
        f.pat_types, f.inputs = dfrac["patTypes"], dfrac["inputs"]
        f.target_classes, f.targets = dfrac.get("targetClasses"), dfrac.get("targets")
        return f

    def prefetch_sequences_resident(self, dfrac):
        """cn_fraction_prefetch_resident: `dfrac` is what the next load_sequences_resident will load; it is re-laid out
        beside the coming backward pass."""
        f = self._resident_descriptor(dfrac)
        B.check(self.lib.cn_fraction_prefetch_resident(self.ctx, self.layers[0].handle, self.layers[-1].handle,
                                                       C.byref(f)), self.ctx)

    def load_sequences_resident(self, dfrac):
        """Like load_sequences, but `dfrac` holds DEVICE pointers (ints) for inputs / patTypes /
        targetClasses / targets: the fraction is already resident in HBM."""
        f = self._resident_descriptor(dfrac)
        B.check(self.lib.cn_fraction_load_resident(self.ctx, self.layers[0].handle, self.layers[-1].handle,
                                                   C.byref(f)), self.ctx)
        self._set_current(f)

    def loss_accumulate(self):
        """Add this fraction's error / #correct to the device-side epoch sums (no host sync)."""
        B.check(self.lib.cn_loss_accumulate(self.layers[-1].handle), self.ctx)

    def loss_read(self, reset=True):
        err, cor = C.c_float(), C.c_int64()
        B.check(self.lib.cn_loss_read(self.ctx, C.byref(err), C.byref(cor), 1 if reset else 0), self.ctx)
        return float(err.value), int(cor.value)

    def ctc_decode(self):
        """cn_ctc_decode: best-path decoding of the current forward pass of a ctc net.  Returns (one int array of labels per sequence
        of the fraction, distances): the Levenshtein distance of each to its label sequence, or None when the fraction has no
        labels."""
        post = self.layers[-1]
        S = getattr(self, "_num_seqs", self.PS)
        T = post.time()[0] if self.T else 1                             # (before a load the call itself says what is wrong)
        dec, lens, dist = np.zeros((S, T), np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        B.check(self.lib.cn_ctc_decode(post.handle, vp(dec), vp(lens), vp(dist)), self.ctx)
        seqs = [dec[s, :lens[s]].copy() for s in range(S)]
        return seqs, (None if S and (dist < 0).all() else dist)

    def ctc_decode_accumulate(self):
        """cn_ctc_decode_accumulate: add this fraction's label errors and label count to the device-side sums (no host sync)."""
        B.check(self.lib.cn_ctc_decode_accumulate(self.layers[-1].handle), self.ctx)

    def ctc_decode_stats(self, reset=True):
        """cn_ctc_decode_read: (label_errors, labels) accumulated so far."""
        e, n = C.c_int64(), C.c_int64()
        B.check(self.lib.cn_ctc_decode_read(self.ctx, C.byref(e), C.byref(n), 1 if reset else 0), self.ctx)
        return int(e.value), int(n.value)

    def compute_forward_pass(self):                                                    # NeuralNetwork.cpp:168-173
        for lay in self.layers:
            B.check(self.lib.cn_layer_forward(lay.handle), self.ctx)

    def compute_backward_pass(self):                                                   # NeuralNetwork.cpp:175-184
        for lay in reversed(self.layers):
            B.check(self.lib.cn_layer_backward(lay.handle), self.ctx)

    def compute_backward_pass_allreduce(self, dist, torch):
        """Backward pass with the data-parallel gradient exchange folded in (SURVEY.md 8e "Overlap", bucket = layer):
        as soon as the backward pass of a layer is enqueued, its weightUpdates (whose gradient GEMMs run on the
        library's side stream) are all-reduced asynchronously from a communication stream that waits for that
        layer's gradient work only (cn_layer_join_stream), i.e. beside the recurrent kernels of the layers below
        it; only the first layer's exchange is exposed.  Returns after every reduction has been ordered before the
        context's stream; follow with update_weights_fused()."""
        if getattr(self, "_comm_stream", None) is None:
            self._comm_stream = torch.cuda.Stream(device=self.device)
        works = []
        main = self.torch_stream(torch)
        for lay in reversed(self.layers):
            B.check(self.lib.cn_layer_backward(lay.handle), self.ctx)
            if lay.trainable:
                B.check(self.lib.cn_layer_join_stream(lay.handle, C.c_void_p(self._comm_stream.cuda_stream)), self.ctx)
                with torch.cuda.stream(self._comm_stream):
                    works.append(dist.all_reduce(lay.weight_updates_tensor(torch), op=dist.ReduceOp.SUM, async_op=True))
        with torch.cuda.stream(main):
            for w in works:
                w.wait()            # orders the context's stream behind the reduction

    # -- data-parallel training through the library's own RCCL communicator -----------------------
    def set_option(self, name, value):
        """cn_ctx_set_option: named integer options of the context ("deterministic": fixed-order gradient sums)."""
        B.check(self.lib.cn_ctx_set_option(self.ctx, name.encode(), int(value)), self.ctx)

    def get_option(self, name):
        v = C.c_int()
        B.check(self.lib.cn_ctx_get_option(self.ctx, name.encode(), C.byref(v)), self.ctx)
        return v.value

    def comm_unique_id(self):
        """Rank 0: 128 rendezvous bytes (ncclGetUniqueId) to hand to every rank out of band."""
        buf = C.create_string_buffer(B.COMM_ID_BYTES)
        B.check(self.lib.cn_comm_unique_id(buf), self.ctx)
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """Collective: bind an RCCL communicator for this context's GPU (cn_comm_init)."""
        if len(unique_id) != B.COMM_ID_BYTES:
            raise ValueError("unique id must be %d bytes" % B.COMM_ID_BYTES)
        B.check(self.lib.cn_comm_init(self.ctx, unique_id, int(rank), int(world)), self.ctx)

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        B.check(self.lib.cn_comm_info(self.ctx, C.byref(r), C.byref(w)), self.ctx)
        return r.value, w.value

    def comm_backend(self):
        """(name, exchanges): which exchange the bound communicator runs ("rccl", "p2p", "ipc"; "" without one) and how many
        all-reduces cn_allreduce_grads has enqueued on it (cn_comm_backend)."""
        k = C.c_int64()
        name = self.lib.cn_comm_backend(self.ctx, C.byref(k))
        return (name or b"").decode(), k.value

    def allreduce_grads(self, layers=None):
        """SUM all-reduce of the weightUpdates of `layers` (None: the whole arena in one exchange) on the library's
        communication stream; the next update waits for it on the device."""
        if not layers:
            B.check(self.lib.cn_allreduce_grads(self.ctx, None, 0), self.ctx)
            return
        arr = (C.c_void_p * len(layers))(*[l.handle for l in layers])
        B.check(self.lib.cn_allreduce_grads(self.ctx, arr, len(layers)), self.ctx)

    def compute_backward_pass_dp(self):
        """Backward pass with the gradient exchange folded in, bucket = layer (SURVEY.md 8e "Overlap"): the reduction of
        layer k is enqueued as soon as its backward pass is, and runs beside the recurrent kernels of the layers below.
        All RCCL calls are made by the library (cn_allreduce_grads); follow with update_weights_fused()."""
        for lay in reversed(self.layers):
            B.check(self.lib.cn_layer_backward(lay.handle), self.ctx)
            if lay.trainable:
                self.allreduce_grads([lay])

    def loss_read_global(self, reset=True):
        err, cor = C.c_float(), C.c_int64()
        B.check(self.lib.cn_loss_read_global(self.ctx, C.byref(err), C.byref(cor), 1 if reset else 0), self.ctx)
        return float(err.value), int(cor.value)

    def recurrent_kernel(self, backward):
        """Name of the recurrent kernel the first LSTM layer launches (for bench.py's roofline record)."""
        for lay in self.layers:
            if lay.type in ("lstm", "blstm"):
                return self.lib.cn_layer_recurrent_kernel(lay.handle, 1 if backward else 0).decode()
        return ""

    def prefetch_hits(self):
        """Loads that found their fraction announced and re-laid out ahead (cn_dbg_prefetch_hits)."""
        n = C.c_int(0)
        B.check(self.lib.cn_dbg_prefetch_hits(self.ctx, C.byref(n)), self.ctx)
        return n.value

    def row_map_counts(self):
        """(computed frames, dummy frames, T x padded parallel sequences) of the loaded fraction's row map (cn_dbg_row_map_counts)."""
        out = (C.c_int * 3)()
        B.check(self.lib.cn_dbg_row_map_counts(self.ctx, out), self.ctx)
        return tuple(out)

    def bf16_preactivation_layers(self):
        """Names of the LSTM layers whose input projection hands its pre-activations to the recurrent kernel as bf16
        (CN_PREC_BF16 with option pre16, the two-sequence forward kernels; LstmRec::pre16) -- as of the LAST forward pass, read off the kernel the
        library reports per layer.  (The parity tests model the rounding of exactly those layers.)"""
        out = []
        if self.precision != B.PREC_BF16:
            return out
        for lay in self.layers:
            if lay.type in ("lstm", "blstm"):
                k = self.lib.cn_layer_recurrent_kernel(lay.handle, 0).decode()
                if "_s2_" in k and self.get_option("pre16") == 1:
                    out.append(lay.name)
        return out

    def _loss(self):
        err, cor = C.c_float(), C.c_int()
        B.check(self.lib.cn_loss_eval(self.layers[-1].handle, C.byref(err), C.byref(cor)), self.ctx)
        return float(err.value), int(cor.value)

    def calculate_error(self):                                                         # NeuralNetwork.cpp:186-190
        return self._loss()[0]

    def count_correct_classifications(self):
        return self._loss()[1]

    def error_and_correct(self):
        return self._loss()

    def update_weights(self, learning_rate, momentum):                                 # SteepestDescentOptimizer.cu:67-94
        for lay in self.trainable_layers():
            lr = lay.learning_rate if lay.learning_rate >= 0.0 else learning_rate
            B.check(self.lib.cn_sgd_update(lay.handle, lr, momentum), self.ctx)

    def arm_update(self, learning_rate, momentum):
        """cn_ctx_arm_update: the coming backward pass applies each layer's momentum-SGD step as soon as that layer's gradient is
        complete; follow the backward pass with update_weights_fused(same values) (or update_weights), which completes the step."""
        B.check(self.lib.cn_ctx_arm_update(self.ctx, learning_rate, momentum), self.ctx)

    def update_weights_fused(self, learning_rate, momentum):
        """One launch for all layers; layers with a JSON learningRate of their own keep it (cn_layer_set_learning_rate)."""
        B.check(self.lib.cn_sgd_update_all(self.ctx, learning_rate, momentum), self.ctx)

    def update_weights_adam(self, learning_rate, beta1=0.9, beta2=0.999, eps=1e-8, step=1, per_layer=False):
        """The Adam step of include/currennt_hip.h (cn_adam_update_all; per_layer: cn_adam_update layer by layer).  `step` is the
        caller's update count, from 1.  Layers with a JSON learningRate of their own keep it."""
        if not per_layer:
            B.check(self.lib.cn_adam_update_all(self.ctx, learning_rate, beta1, beta2, eps, int(step)), self.ctx)
            return
        for lay in self.trainable_layers():
            lr = lay.learning_rate if lay.learning_rate >= 0.0 else learning_rate
            B.check(self.lib.cn_adam_update(lay.handle, lr, beta1, beta2, eps, int(step)), self.ctx)

    def arm_adam(self, learning_rate, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        """cn_ctx_arm_adam: the coming backward pass applies each layer's Adam step as soon as that layer's gradient is complete;
        follow the backward pass with update_weights_adam(same values), which completes the step."""
        B.check(self.lib.cn_ctx_arm_adam(self.ctx, learning_rate, beta1, beta2, eps, int(step)), self.ctx)

    def update_weights_lamb(self, learning_rate, beta1=0.9, beta2=0.999, eps=1e-8, step=1, per_layer=False):
        """The LAMB step of include/currennt_hip.h (cn_lamb_update_all; per_layer: cn_lamb_update layer by layer).  `step` is the
        caller's update count, from 1.  Layers with a JSON learningRate of their own keep it."""
        if not per_layer:
            B.check(self.lib.cn_lamb_update_all(self.ctx, learning_rate, beta1, beta2, eps, int(step)), self.ctx)
            return
        for lay in self.trainable_layers():
            lr = lay.learning_rate if lay.learning_rate >= 0.0 else learning_rate
            B.check(self.lib.cn_lamb_update(lay.handle, lr, beta1, beta2, eps, int(step)), self.ctx)

    def arm_lamb(self, learning_rate, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        """cn_ctx_arm_lamb: accepted and checked; update_weights_lamb(same values) behind the backward pass applies the step."""
        B.check(self.lib.cn_ctx_arm_lamb(self.ctx, learning_rate, beta1, beta2, eps, int(step)), self.ctx)

    def set_trust_bounds(self, min_ratio, max_ratio):
        """cn_ctx_set_trust_bounds: the bounds of every layer's LAMB trust ratio; max_ratio 0 means no upper bound."""
        B.check(self.lib.cn_ctx_set_trust_bounds(self.ctx, float(min_ratio), float(max_ratio)), self.ctx)

    def trust_bounds(self):
        """cn_ctx_get_trust_bounds: (min_ratio, max_ratio) as np.float32."""
        a, b = C.c_float(), C.c_float()
        B.check(self.lib.cn_ctx_get_trust_bounds(self.ctx, C.byref(a), C.byref(b)), self.ctx)
        return np.float32(a.value), np.float32(b.value)

    def average_weights(self, decay):
        """cn_ctx_average_weights: one step avg += (1 - decay) * (w - avg) over all weights, behind the update that precedes it
        (include/currennt_hip.h, section Weight averaging); the context's first step copies.  The library keeps no clock: a
        training loop hands the decay of each step."""
        B.check(self.lib.cn_ctx_average_weights(self.ctx, float(decay)), self.ctx)

    def swap_weight_average(self):
        """cn_ctx_swap_weight_average: exchange the weights and their average; the forward passes that follow read the average
        until the next call swaps them back.  Nothing may train or update in between."""
        B.check(self.lib.cn_ctx_swap_weight_average(self.ctx), self.ctx)

    def weight_average_state(self):
        """cn_ctx_weight_average_state: (exists, swapped)."""
        e, s = C.c_int(), C.c_int()
        B.check(self.lib.cn_ctx_weight_average_state(self.ctx, C.byref(e), C.byref(s)), self.ctx)
        return bool(e.value), bool(s.value)

    def set_dropout_pass(self, enable, seed=0, pass_=0):
        """cn_ctx_set_dropout_pass: whether the forward passes that follow drop (on the layers with a "dropout" rate), and the
        64-bit (seed, pass) of their masks.  The library keeps no clock: a training loop hands a new pass per fraction."""
        B.check(self.lib.cn_ctx_set_dropout_pass(self.ctx, 1 if enable else 0, int(seed) & (2 ** 64 - 1), int(pass_) & (2 ** 64 - 1)), self.ctx)

    def set_weight_noise(self, sigma, seed=0, pass_=0):
        """cn_ctx_set_weight_noise: the backward passes that follow read w + N(0, sigma^2) noise generated on the device from the
        64-bit (seed, pass) (include/currennt_hip.h, section Weight noise); the forward pass and the update keep the clean weights.
        sigma 0 turns it off.  The library keeps no clock: a training loop hands a new pass per fraction."""
        B.check(self.lib.cn_ctx_set_weight_noise(self.ctx, float(sigma), int(seed) & (2 ** 64 - 1), int(pass_) & (2 ** 64 - 1)), self.ctx)

    def set_input_augment(self, noise_sigma=0.0, context=(0, 0), freq_masks=0, freq_width=0, time_masks=0, time_width=0,
                          time_max_permille=1000, seed=0, pass_=0):
        """cn_ctx_set_input_augment: the loads (and prefetches) that follow re-lay their fraction out with Gaussian input noise and
        SpecAugment masks generated on the device from the 64-bit (seed, pass) (include/currennt_hip.h, section Input
        augmentation); `context` = (left, right) is how the caller spliced the patterns.  set_input_augment(None), or no noise and
        no masks, turns it off.  The library keeps no clock: a training loop hands a new pass per fraction."""
        if noise_sigma is None:
            B.check(self.lib.cn_ctx_set_input_augment(self.ctx, None), self.ctx)
            return
        a = B.InputAugment(float(noise_sigma), int(context[0]), int(context[1]), int(freq_masks), int(freq_width), int(time_masks),
                           int(time_width), int(time_max_permille), int(seed) & (2 ** 64 - 1), int(pass_) & (2 ** 64 - 1))
        B.check(self.lib.cn_ctx_set_input_augment(self.ctx, C.byref(a)), self.ctx)

    def set_input_splice(self, context=(0, 0), frame_skip=1):
        """cn_ctx_set_input_splice: the loads (and prefetches) that follow take a fraction built WITHOUT context at source rate
        (make_fraction(xs, ts, PS)); the device splices `context` = (left, right) neighbouring frames into each pattern and keeps
        every frame_skip-th frame (include/currennt_hip.h, section Input splicing and frame skipping).  Every read-back is then
        sized by ceil(T / frame_skip).  set_input_splice(None) turns it off; (0, 0) with frame_skip 1 is on, the identity."""
        if context is None:
            B.check(self.lib.cn_ctx_set_input_splice(self.ctx, None), self.ctx)
            self.frame_skip = 1
            return
        s = B.InputSplice(int(context[0]), int(context[1]), int(frame_skip))
        B.check(self.lib.cn_ctx_set_input_splice(self.ctx, C.byref(s)), self.ctx)
        self.frame_skip = int(frame_skip)

    def set_grad_clip(self, max_norm):
        """cn_ctx_set_grad_clip: clip every update's gradient to this global L2 norm (include/currennt_hip.h, section Gradient
        clipping); 0 turns it off, a bound nothing reaches (FLT_MAX) only monitors the norm."""
        B.check(self.lib.cn_ctx_set_grad_clip(self.ctx, float(max_norm)), self.ctx)

    def grad_clip_stats(self, reset=False):
        """cn_ctx_grad_clip_stats: dict(last_norm, last_scale, updates, clipped, skipped, max_norm_seen); zeros with clipping off."""
        f = [C.c_float() for _ in range(3)]
        n = [C.c_int64() for _ in range(3)]
        B.check(self.lib.cn_ctx_grad_clip_stats(self.ctx, C.byref(f[0]), C.byref(f[1]), C.byref(n[0]), C.byref(n[1]), C.byref(n[2]),
                                                C.byref(f[2]), 1 if reset else 0), self.ctx)
        return dict(last_norm=np.float32(f[0].value), last_scale=np.float32(f[1].value), updates=n[0].value, clipped=n[1].value,
                    skipped=n[2].value, max_norm_seen=np.float32(f[2].value))

    def set_weight_decay(self, decay):
        """cn_ctx_set_weight_decay: decoupled weight decay of the updates that follow (include/currennt_hip.h, section Weight
        decay): every input and recurrent weight shrinks by lr * decay of itself in front of the optimizer's step; 0 turns it off."""
        B.check(self.lib.cn_ctx_set_weight_decay(self.ctx, float(decay)), self.ctx)

    def weight_decay(self):
        """cn_ctx_get_weight_decay: the coefficient in force (np.float32)."""
        d = C.c_float()
        B.check(self.lib.cn_ctx_get_weight_decay(self.ctx, C.byref(d)), self.ctx)
        return np.float32(d.value)

    def accumulate_updates(self, first):
        """Batch learning (Optimizer.cu:72-85): add this fraction's weightUpdates of all layers to the epoch sum on the device
        (`first`: copy instead of add)."""
        B.check(self.lib.cn_ctx_accumulate_updates(self.ctx, 1 if first else 0), self.ctx)

    def take_accumulated(self):
        """The epoch sum becomes every layer's weightUpdates again (in front of the one update of the epoch, :95-97)."""
        B.check(self.lib.cn_ctx_take_accumulated(self.ctx), self.ctx)

    def outputs(self):
        """Output layer activations [T][PS][C] (NeuralNetwork.cpp:237-262 de-interleaves per sequence); T of the output layer's
        own time axis."""
        return self.output_layer().outputs()

    def lengths(self, layer=None):
        """The real frames per sequence slot of the fraction loaded last as `layer` (default: the input layer) sees them:
        n_s = ceil(len_s / rate) (include/currennt_hip.h, section Strided context layers)."""
        lay = self.layers[0] if layer is None else (self.layer(layer) if isinstance(layer, str) else layer)
        if self._lens is None and self._lens_from is not None:
            pat, T, k = self._lens_from
            self._lens = -(-(np.asarray(pat).reshape(T, -1) != 0).sum(axis=0).astype(np.int64) // k)
        if self._lens is None:
            self._lens = (self.axis(self.layers[0])[0][:, :self.PS] != 0).sum(axis=0).astype(np.int64)
        return -(-self._lens // lay.rate)

    def axis(self, layer):
        """(patTypes [T'][PSp], classes [T'][PSp], lengths [PSp]) of the time axis `layer` runs on, as the device holds them
        (cn_dbg_layer_axis; pad slots included)."""
        lay = self.layer(layer) if isinstance(layer, str) else layer
        psp = C.c_int()
        B.check(self.lib.cn_dbg_layer_axis(lay.handle, None, None, None, 0, C.byref(psp)), self.ctx)
        rows = lay.T * psp.value
        pat, cls, ln = np.empty(rows, np.int8), np.empty(rows, np.int32), np.empty(psp.value, np.int32)
        has_len = any(l.type == "context" for l in self.layers)
        B.check(self.lib.cn_dbg_layer_axis(lay.handle, pat.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p),
                                           ln.ctypes.data_as(C.c_void_p) if has_len else None, rows, None), self.ctx)
        return pat.reshape(lay.T, psp.value), cls.reshape(lay.T, psp.value), (ln if has_len else None)

    def torch_stream(self, torch):
        """The context's HIP stream as a torch stream.  Collectives and tensor ops that must be ordered against the
        library's work run under `with torch.cuda.stream(net.torch_stream(torch))` -- torch's current stream is NOT the
        context's stream unless the caller made it so (a default-stream handle of 0 given to the constructor means
        "library-owned stream")."""
        if getattr(self, "_torch_stream", None) is None:
            self._torch_stream = torch.cuda.ExternalStream(int(self.lib.cn_ctx_stream(self.ctx)), device=torch.device("cuda", self.device))
        return self._torch_stream

    def join(self):
        """Order the ctx stream behind the internal side stream (before an external all-reduce)."""
        B.check(self.lib.cn_ctx_join(self.ctx), self.ctx)

    def synchronize(self):
        B.check(self.lib.cn_ctx_synchronize(self.ctx), self.ctx)

    def param_arena(self):
        """(weights_ptr, weight_updates_ptr, weight_deltas_ptr, count) raw device pointers."""
        w, g, d, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        B.check(self.lib.cn_ctx_param_arena(self.ctx, C.byref(w), C.byref(g), C.byref(d), C.byref(n)), self.ctx)
        return w.value, g.value, d.value, n.value

    def export_weights(self):
        """The "weights" JSON section (TrainableLayer.cu:211-248: input / bias / internal)."""
        out = {}
        for lay in self.trainable_layers():
            w = lay.weights()
            P, L = lay.prev.size, lay.size
            per_in = 4 if lay.type in ("lstm", "blstm") else 1
            n_in, n_b = L * per_in * P, L * per_in
            out[lay.name] = {"input": w[:n_in].tolist(), "bias": w[n_in:n_in + n_b].tolist(),
                             "internal": w[n_in + n_b:].tolist()}
        return out

    # -- timing ---------------------------------------------------------------------------------
    def timing_enable(self, on=True):
        B.check(self.lib.cn_ctx_timing_enable(self.ctx, 1 if on else 0), self.ctx)

    def timing_reset(self):
        B.check(self.lib.cn_ctx_timing_reset(self.ctx), self.ctx)

    def timing_read(self):
        names = ["rec_fwd", "rec_bwd", "gemm_wide", "gemm_grad", "other", "exchange"]
        out = {}
        for k, nm in enumerate(names):
            ms, n = C.c_double(), C.c_int64()
            B.check(self.lib.cn_ctx_timing_read(self.ctx, k, C.byref(ms), C.byref(n)), self.ctx)
            out[nm] = (ms.value, n.value)
        return out
