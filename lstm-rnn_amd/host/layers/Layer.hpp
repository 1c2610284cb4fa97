// Layer objects of the host side: same class roles, method names and error texts as
// currennt_lib/src/layers/{Layer,TrainableLayer,InputLayer,LstmLayer,FeedForwardLayer,SoftmaxLayer,
// PostOutputLayer,SsePostOutputLayer,MulticlassClassificationLayer}.hpp for the `Hip` device policy.
// Every compute method is one call into the C ABI (include/currennt_hip.h); vectors returned by
// outputs()/weights()/... are host copies in the reference layouts.
#pragma once

#include <string>
#include <vector>

#include "../Json.hpp"
#include "../Types.hpp"
#include "../data_sets/DataSet.hpp"

namespace currennt_hip {
namespace layers {

class Layer {                                             // layers/Layer.hpp:40-179
public:
    Layer(cn_ctx *ctx, const json::Value &layerChild, cn_layer_kind kind, Layer *precedingLayer,
          int parallelSequences, int maxSeqLength, float bias);
    virtual ~Layer();

    const std::string &name() const { return m_name; }
    int size() const { return m_size; }
    int parallelSequences() const { return m_parallelSequences; }
    int maxSeqLength() const { return m_maxSeqLength; }
    int curMaxSeqLength() const { return m_curMaxSeqLength; }
    int curMinSeqLength() const { return m_curMinSeqLength; }
    int curNumSeqs() const { return m_curNumSeqs; }
    // the product of the strides of the context layers in front of (and of) this layer: its lengths, pattern types and read-backs
    // go by ceil(network-rate length / rate) (include/currennt_hip.h, section Strided context layers)
    int rate() const { return m_rate; }
    // (behind a strided context layer: that layer's vector, one per time axis)
    const Hip::pattype_vector &patTypes() const { return m_axisOwner && m_axisOwner != this ? m_axisOwner->m_patTypes : m_patTypes; }
    virtual const std::string &type() const = 0;
    virtual bool isTrainable() const { return false; }
    virtual bool isPostOutput() const { return false; }
    bool residual() const { return m_residual; }          // JSON "residual": followers read this layer's output plus its input

    bool layerNorm() const { return m_layerNorm; }        // JSON "layer_norm": this layer's input products read a normalised copy of its input
    float layerNormEps() const { return m_layerNormEps; } // JSON "layer_norm_eps"

    Hip::real_vector outputs() const;                     // Layer.hpp:132
    Hip::real_vector outputErrors() const;                // Layer.hpp:153

    virtual void loadSequences(const data_sets::DataSetFraction &fraction);   // Layer.cpp:134-141
    virtual void computeForwardPass();
    virtual void computeBackwardPass();
    virtual void exportLayer(json::Value *layersArray) const;                 // Layer.cpp:143-157

    cn_layer *handle() const { return m_handle; }
    cn_ctx *context() const { return m_ctx; }

    // "left", "right", "dilation" and "stride" of a "context" layer description, each absent or an integer in its range; a value
    // that is not is refused with a message that names the layer.  Needs no device: a network file is held to it before one is
    // touched.
    static void contextMemberValues(const json::Value &layerChild, const std::string &name, int values[4]);

protected:
    Hip::real_vector read(cn_buffer which, int dir, size_t count) const;
    // the members of a "context" layer description, checked: the constructor below creates such a layer from them
    static void contextMembers(const json::Value &layerChild, const std::string &name, int size, const Layer *precedingLayer,
                               int *left, int *right, int *dilation, int *stride);

    cn_ctx *m_ctx;
    cn_layer *m_handle;
    std::string m_name;
    int m_size;
    int m_parallelSequences, m_maxSeqLength, m_curMaxSeqLength, m_curMinSeqLength, m_curNumSeqs;
    int m_rate;
    const Layer *m_axisOwner;         // the nearest strided context layer in front of (or this) layer: it holds the axis's pattern types; 0: none
    Hip::pattype_vector m_patTypes;
    bool m_residual;
    bool m_layerNorm;
    float m_layerNormEps;
};

class InputLayer : public Layer {                         // layers/InputLayer.{hpp,cpp}
public:
    InputLayer(cn_ctx *ctx, const json::Value &layerChild, int parallelSequences, int maxSeqLength);
    const std::string &type() const;
    void loadSequences(const data_sets::DataSetFraction &fraction);
};

// A hidden layer without weights that splices its preceding layer's neighbouring frames (include/currennt_hip.h, section Context
// layers; no counterpart in the reference): JSON "left" / "right" (default 0) frames at steps of "dilation" (default 1), and a
// "size" of (left + right + 1) x the preceding layer's size; "stride" (default 1) keeps every stride-th frame (section Strided
// context layers)
class ContextLayer : public Layer {
public:
    ContextLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
    int left() const { return m_left; }
    int right() const { return m_right; }
    int dilation() const { return m_dilation; }
    int stride() const { return m_stride; }
    void exportLayer(json::Value *layersArray) const;
private:
    int m_left, m_right, m_dilation, m_stride;
};

class TrainableLayer : public Layer {                     // layers/TrainableLayer.{hpp,cu}
public:
    TrainableLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, cn_layer_kind kind,
                   int inputWeightsPerBlock, int internalWeightsPerBlock, Layer &precedingLayer);
    bool isTrainable() const { return true; }
    Layer &precedingLayer() { return m_precedingLayer; }
    const Layer &precedingLayer() const { return m_precedingLayer; }
    real_t bias() const { return m_bias; }
    real_t learningRate() const { return m_learningRate; }
    real_t dropout() const { return m_dropout; }        // JSON "dropout": rate of the dropout on this layer's input (0: none)
    Hip::real_vector weights() const;                     // TrainableLayer.hpp:119
    Hip::real_vector weightUpdates() const;               // TrainableLayer.hpp:133
    void setWeights(const Hip::real_vector &w);
    int weightCount() const;
    void exportWeights(json::Value *weightsObject) const; // TrainableLayer.cu:211-248
    void exportLayer(json::Value *layersArray) const;     // TrainableLayer.cu:250-255

private:
    Layer &m_precedingLayer;
    int m_inputWeightsPerBlock, m_internalWeightsPerBlock;
    real_t m_bias, m_learningRate, m_dropout;
};

class FeedForwardLayer : public TrainableLayer {          // layers/FeedForwardLayer.{hpp,cu}
public:
    FeedForwardLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer,
                     cn_layer_kind kind);
    const std::string &type() const;
private:
    std::string m_type;
};

class SoftmaxLayer : public TrainableLayer {              // layers/SoftmaxLayer.{hpp,cu}
public:
    SoftmaxLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer);
    const std::string &type() const;
};

class LstmLayer : public TrainableLayer {                 // layers/LstmLayer.{hpp,cu}
public:
    LstmLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer, bool bidirectional);
    const std::string &type() const;
    bool isBidirectional() const { return m_isBidirectional; }
    // the ten per-direction vectors of LstmLayer.hpp:170-233; unlike the reference they are also
    // available for bidirectional layers (direction 0 = forward states, 1 = backward states)
    Hip::real_vector cellStates(int dir = 0) const { return internal(CN_BUF_LSTM_CELL_STATES, dir); }
    Hip::real_vector netInputActs(int dir = 0) const { return internal(CN_BUF_LSTM_NI_ACTS, dir); }
    Hip::real_vector inputGateActs(int dir = 0) const { return internal(CN_BUF_LSTM_IG_ACTS, dir); }
    Hip::real_vector forgetGateActs(int dir = 0) const { return internal(CN_BUF_LSTM_FG_ACTS, dir); }
    Hip::real_vector outputGateActs(int dir = 0) const { return internal(CN_BUF_LSTM_OG_ACTS, dir); }
    Hip::real_vector netInputDeltas(int dir = 0) const { return internal(CN_BUF_LSTM_NI_DELTAS, dir); }
    Hip::real_vector inputGateDeltas(int dir = 0) const { return internal(CN_BUF_LSTM_IG_DELTAS, dir); }
    Hip::real_vector forgetGateDeltas(int dir = 0) const { return internal(CN_BUF_LSTM_FG_DELTAS, dir); }
    Hip::real_vector outputGateDeltas(int dir = 0) const { return internal(CN_BUF_LSTM_OG_DELTAS, dir); }
private:
    Hip::real_vector internal(cn_buffer which, int dir) const;
    bool m_isBidirectional;
};

class PostOutputLayer : public Layer {                    // layers/PostOutputLayer.{hpp,cpp}
public:
    PostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, cn_layer_kind kind, Layer &precedingLayer);
    bool isPostOutput() const { return true; }
    void loadSequences(const data_sets::DataSetFraction &fraction);
    virtual real_t calculateError();                      // PostOutputLayer.hpp:80
    virtual int countCorrectClassifications() { return -1; }
protected:
    Layer &m_precedingLayer;
};

class SsePostOutputLayer : public PostOutputLayer {       // layers/SsePostOutputLayer.{hpp,cu}
public:
    SsePostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
};

class MulticlassClassificationLayer : public PostOutputLayer {   // layers/MulticlassClassificationLayer.{hpp,cu}
public:
    MulticlassClassificationLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
    int countCorrectClassifications();
};

// Connectionist Temporal Classification (no counterpart in the reference): behind a softmax layer of numLabels + 1 units, the
// last one the blank; trains against the fraction's label sequences (DataSetFraction::labelSeqs)
class CtcPostOutputLayer : public PostOutputLayer {
public:
    CtcPostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
    void loadSequences(const data_sets::DataSetFraction &fraction);
    void setLabelSequences(const data_sets::DataSetFraction &fraction);     // behind cn_fraction_load: cn_layer_set_label_sequences
    int countCorrectClassifications();                                      // sequences that contributed to the error
};

// The remaining post output layers of LayerFactory.cu:52-87; each is a thin handle on the C ABI kind.
class WeightedSsePostOutputLayer : public PostOutputLayer {   // layers/WeightedSsePostOutputLayer.{hpp,cu}; size = 2 x output layer
public:
    WeightedSsePostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
};
class SseMaskPostOutputLayer : public PostOutputLayer {       // layers/SseMaskPostOutputLayer.{hpp,cu} ("wf"); size = 2 x output layer
public:
    SseMaskPostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
};
class CePostOutputLayer : public PostOutputLayer {            // layers/CePostOutputLayer.{hpp,cu}
public:
    CePostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
};
class RmsePostOutputLayer : public PostOutputLayer {          // layers/RmsePostOutputLayer.{hpp,cu}
public:
    RmsePostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
};
class BinaryClassificationLayer : public PostOutputLayer {    // layers/BinaryClassificationLayer.{hpp,cu}
public:
    BinaryClassificationLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer);
    const std::string &type() const;
    int countCorrectClassifications();
};

}  // namespace layers
}  // namespace currennt_hip
