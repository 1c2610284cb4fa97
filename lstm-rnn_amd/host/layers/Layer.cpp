#include "Layer.hpp"

#include <cmath>
#include <stdexcept>

namespace currennt_hip {
namespace layers {

namespace {
float jsonBias(const json::Value &layerChild) { return layerChild.hasMember("bias") ? (float)layerChild["bias"].getDouble() : 0.f; }
}

// ---- Layer ----------------------------------------------------------------------------------
Layer::Layer(cn_ctx *ctx, const json::Value &layerChild, cn_layer_kind kind, Layer *precedingLayer,
             int parallelSequences, int maxSeqLength, float bias)
    : m_ctx(ctx), m_handle(0)
    , m_name(layerChild.hasMember("name") ? layerChild["name"].getString() : "")
    , m_size(layerChild.hasMember("size") ? layerChild["size"].getInt() : 0)
    , m_parallelSequences(parallelSequences), m_maxSeqLength(maxSeqLength)
    , m_curMaxSeqLength(0), m_curMinSeqLength(0), m_curNumSeqs(0), m_rate(precedingLayer ? precedingLayer->rate() : 1), m_axisOwner(precedingLayer ? precedingLayer->m_axisOwner : 0), m_residual(false), m_layerNorm(false), m_layerNormEps(1e-5f)
{
    if (!layerChild.hasMember("name")) throw std::runtime_error("Missing value 'name' in layer description");       // Layer.cpp:52-53
    if (m_name.empty()) throw std::runtime_error("Empty layer name in layer description");                           // :54-55
    if (!layerChild.hasMember("size")) throw std::runtime_error("Missing value 'size' in layer '" + m_name + "'");  // :56-57
    // "dropout" acts on a trainable layer's input (TrainableLayer reads it): on an input or post output layer it is an error, not
    // a member to ignore (the Python mirror refuses the same file)
    const bool trainableKind = kind == CN_LAYER_LSTM || kind == CN_LAYER_BLSTM || kind == CN_LAYER_FF_TANH || kind == CN_LAYER_FF_LOGISTIC ||
                               kind == CN_LAYER_FF_IDENTITY || kind == CN_LAYER_SOFTMAX;
    if (layerChild.hasMember("dropout") && !trainableKind)
        throw std::runtime_error("Invalid value 'dropout' in layer '" + m_name + "': only lstm, blstm, feedforward_* and softmax layers take dropout");
    // "residual": true marks a hidden layer whose followers read its output plus its input (include/currennt_hip.h, section
    // Residual connections; the reference has none).  The three refusals are the library's, said here with the layer's name.
    if (layerChild.hasMember("residual")) {
        const bool residualKind = trainableKind && kind != CN_LAYER_SOFTMAX;
        if (layerChild["residual"].type() != json::Value::Bool)
            throw std::runtime_error("Invalid value 'residual' in layer '" + m_name + "': true or false expected");
        if (!residualKind)
            throw std::runtime_error("Invalid value 'residual' in layer '" + m_name + "': only lstm, blstm and feedforward_* layers can be residual");
        m_residual = layerChild["residual"].getBool();
        if (m_residual && m_size != precedingLayer->size())
            throw std::runtime_error("Invalid value 'residual' in layer '" + m_name + "': the layer's size " + std::to_string(m_size) +
                                     " differs from the preceding layer's size " + std::to_string(precedingLayer->size()));
    }
    if (precedingLayer && precedingLayer->residual() && !trainableKind && kind != CN_LAYER_CONTEXT)
        throw std::runtime_error("Invalid value 'residual' in layer '" + precedingLayer->name() + "': a post output layer cannot follow a residual layer directly");
    // "layer_norm": true marks a trainable layer whose input products read a normalised copy of its input, "layer_norm_eps" is the
    // eps under the square root (include/currennt_hip.h, section Layer normalization; the reference has none).  The refusals are
    // the library's, said here with the layer's name.
    if (layerChild.hasMember("layer_norm") || layerChild.hasMember("layer_norm_eps")) {
        const std::string member = layerChild.hasMember("layer_norm") ? "layer_norm" : "layer_norm_eps";
        if (!trainableKind)
            throw std::runtime_error("Invalid value '" + member + "' in layer '" + m_name + "': only lstm, blstm, feedforward_* and softmax layers normalise their input");
        if (layerChild.hasMember("layer_norm") && layerChild["layer_norm"].type() != json::Value::Bool)
            throw std::runtime_error("Invalid value 'layer_norm' in layer '" + m_name + "': true or false expected");
        if (layerChild.hasMember("layer_norm_eps")) {
            const json::Value &eps = layerChild["layer_norm_eps"];
            if (!eps.isNumber() || !(eps.getDouble() > 0) || !std::isfinite((float)eps.getDouble()))
                throw std::runtime_error("Invalid value 'layer_norm_eps' in layer '" + m_name + "': a finite number above 0 expected");
            m_layerNormEps = (float)eps.getDouble();
        }
        m_layerNorm = layerChild.hasMember("layer_norm") && layerChild["layer_norm"].getBool();
        if (m_layerNorm && precedingLayer->size() < 2)
            throw std::runtime_error("Invalid value 'layer_norm' in layer '" + m_name + "': the preceding layer's size " +
                                     std::to_string(precedingLayer->size()) + " is below 2");
    }
    if (kind == CN_LAYER_CONTEXT) {        // (a kind with members of its own and an entry point of its own)
        int left, right, dilation, stride;
        contextMembers(layerChild, m_name, m_size, precedingLayer, &left, &right, &dilation, &stride);
        if (stride == 1) hipCheck(cn_layer_create_context(ctx, precedingLayer->handle(), left, right, dilation, &m_handle), ctx);
        else hipCheck(cn_layer_create_context_strided(ctx, precedingLayer->handle(), left, right, dilation, stride, &m_handle), ctx);
        m_rate *= stride;
        if (stride > 1) m_axisOwner = this;
        m_maxSeqLength = (m_maxSeqLength + stride - 1) / stride;
    } else {
        hipCheck(cn_layer_create(ctx, kind, precedingLayer ? precedingLayer->handle() : 0, m_size, bias,
                                 precedingLayer ? 0 : parallelSequences, precedingLayer ? 0 : maxSeqLength, &m_handle), ctx);
    }
    if (m_residual) hipCheck(cn_layer_set_residual(m_handle, 1), ctx);
    if (m_layerNorm) hipCheck(cn_layer_set_layer_norm(m_handle, 1, m_layerNormEps), ctx);
}

Layer::~Layer() {}     // device memory belongs to the context (cn_ctx_destroy)

Hip::real_vector Layer::read(cn_buffer which, int dir, size_t count) const
{
    Hip::real_vector v(count);
    if (count) hipCheck(cn_layer_read(m_handle, which, dir, v.data(), count), m_ctx);
    return v;
}
Hip::real_vector Layer::outputs() const { return read(CN_BUF_OUTPUTS, 0, (size_t)m_curMaxSeqLength * m_parallelSequences * m_size); }
Hip::real_vector Layer::outputErrors() const { return read(CN_BUF_OUTPUT_ERRORS, 0, (size_t)m_curMaxSeqLength * m_parallelSequences * m_size); }

void Layer::loadSequences(const data_sets::DataSetFraction &fraction)
{
    m_curMaxSeqLength = fraction.networkMaxSeqLength();     // (a source-rate fraction: what the device derives from it)
    m_curMinSeqLength = fraction.networkMinSeqLength();
    m_curNumSeqs = fraction.numSequences();
    if (m_rate == 1) { m_patTypes = fraction.networkPatTypes(); return; }
    // behind a strided context layer: the axis the device derives (section Strided context layers)
    m_curMaxSeqLength = (m_curMaxSeqLength + m_rate - 1) / m_rate;
    m_curMinSeqLength = (m_curMinSeqLength + m_rate - 1) / m_rate;
    if (m_axisOwner != this) return;      // (the axis's owner, loaded in front of this layer, holds the pattern types)
    m_patTypes.assign((size_t)m_curMaxSeqLength * m_parallelSequences, PATTYPE_NONE);
    for (int i = 0; i < fraction.numSequences(); ++i) {
        const int n = (fraction.seqInfo(i).length + m_rate - 1) / m_rate;
        for (int j = 0; j < n; ++j)
            m_patTypes[(size_t)j * m_parallelSequences + i] = j == 0 ? PATTYPE_FIRST : (j == n - 1 ? PATTYPE_LAST : PATTYPE_NORMAL);
    }
}
void Layer::computeForwardPass() { hipCheck(cn_layer_forward(m_handle), m_ctx); }
void Layer::computeBackwardPass() { hipCheck(cn_layer_backward(m_handle), m_ctx); }

void Layer::exportLayer(json::Value *layersArray) const
{
    if (!layersArray->isArray()) throw std::runtime_error("The JSON value is not an array");
    json::Value o(json::Value::Object);
    o.addMember("name", name());
    o.addMember("type", type());
    o.addMember("size", size());
    layersArray->pushBack(o);
}

// ---- ContextLayer ---------------------------------------------------------------------------
// The refusals are the library's (include/currennt_hip.h, section Context layers), said here with the layer's name; the size
// check uses the reference's text for a size that does not fit the preceding layer (PostOutputLayer.cpp:58-59).
void Layer::contextMembers(const json::Value &layerChild, const std::string &name, int size, const Layer *precedingLayer,
                           int *left, int *right, int *dilation, int *stride)
{
    int values[4];
    contextMemberValues(layerChild, name, values);
    *left = values[0]; *right = values[1]; *dilation = values[2]; *stride = values[3];
    const int blocks = *left + *right + 1;
    if (size != blocks * precedingLayer->size())
        throw std::runtime_error("Size mismatch: " + std::to_string(size) + " vs. " + std::to_string(blocks * precedingLayer->size()) + " in layer '" + name +
                                 "' (" + std::to_string(blocks) + " frames of the preceding layer's " + std::to_string(precedingLayer->size()) + " units)");
}
void Layer::contextMemberValues(const json::Value &layerChild, const std::string &name, int values[4])
{
    struct Member { const char *key; int dflt, lo, hi; };
    const Member members[4] = {{"left", 0, 0, 32}, {"right", 0, 0, 32}, {"dilation", 1, 1, 16}, {"stride", 1, 1, 8}};
    for (int k = 0; k < 4; ++k) {
        const Member &m = members[k];
        values[k] = m.dflt;
        if (!layerChild.hasMember(m.key)) continue;
        const json::Value &v = layerChild[m.key];
        if (!v.isNumber() || v.getDouble() != std::floor(v.getDouble()) || v.getDouble() < m.lo || v.getDouble() > m.hi)
            throw std::runtime_error(std::string("Invalid value '") + m.key + "' in layer '" + name + "': an integer in " + std::to_string(m.lo) +
                                     ".." + std::to_string(m.hi) + " expected");
        values[k] = v.getInt();
    }
}
ContextLayer::ContextLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer)
    : Layer(ctx, layerChild, CN_LAYER_CONTEXT, &precedingLayer, precedingLayer.parallelSequences(), precedingLayer.maxSeqLength(), 0.f)
    , m_left(0), m_right(0), m_dilation(1), m_stride(1)
{
    hipCheck(cn_layer_context(m_handle, &m_left, &m_right, &m_dilation), ctx);
    hipCheck(cn_layer_context_stride(m_handle, &m_stride), ctx);
}
const std::string &ContextLayer::type() const { static const std::string s("context"); return s; }
void ContextLayer::exportLayer(json::Value *layersArray) const
{
    Layer::exportLayer(layersArray);
    json::Value &o = (*layersArray)[layersArray->size() - 1];
    o.addMember("left", m_left); o.addMember("right", m_right); o.addMember("dilation", m_dilation);
    if (m_stride != 1) o.addMember("stride", m_stride);      // (files of nets without a stride stay as they were)
}

// ---- InputLayer -----------------------------------------------------------------------------
InputLayer::InputLayer(cn_ctx *ctx, const json::Value &layerChild, int parallelSequences, int maxSeqLength)
    : Layer(ctx, layerChild, CN_LAYER_INPUT, 0, parallelSequences, maxSeqLength, 0.f) {}
const std::string &InputLayer::type() const { static const std::string s("input"); return s; }
void InputLayer::loadSequences(const data_sets::DataSetFraction &fraction)
{
    // (a source-rate fraction brings unspliced patterns: the library holds their size to this layer's at the load)
    if (fraction.inputPatternSize() != size() && !fraction.sourceRate())   // InputLayer.cpp:52-55
        throw std::runtime_error("Input layer size of " + std::to_string(size()) + " != data input pattern size of " +
                                 std::to_string(fraction.inputPatternSize()));
    Layer::loadSequences(fraction);
}

// ---- TrainableLayer -------------------------------------------------------------------------
TrainableLayer::TrainableLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, cn_layer_kind kind,
                               int inputWeightsPerBlock, int internalWeightsPerBlock, Layer &precedingLayer)
    : Layer(ctx, layerChild, kind, &precedingLayer, precedingLayer.parallelSequences(), precedingLayer.maxSeqLength(), jsonBias(layerChild))
    , m_precedingLayer(precedingLayer)
    , m_inputWeightsPerBlock(inputWeightsPerBlock), m_internalWeightsPerBlock(internalWeightsPerBlock)
    , m_bias(jsonBias(layerChild))
    , m_learningRate(layerChild.hasMember("learningRate") ? (real_t)layerChild["learningRate"].getDouble() : -1)
    , m_dropout(layerChild.hasMember("dropout") ? (real_t)layerChild["dropout"].getDouble() : 0)
{
    if (!layerChild.hasMember("bias")) throw std::runtime_error("Missing value 'bias' in layer '" + name() + "'");   // TrainableLayer.cu:61-62
    // the layer's own learning rate (TrainableLayer.cu:58) is also what an armed update (cn_ctx_arm_update) applies to it
    if (m_learningRate >= 0) cn_layer_set_learning_rate(m_handle, m_learningRate);
    // dropout on this layer's input (include/currennt_hip.h, section Dropout; the reference has none)
    if (!(m_dropout >= 0 && m_dropout < 1)) throw std::runtime_error("Invalid value 'dropout' in layer '" + name() + "': the rate must lie in [0, 1)");
    if (m_dropout > 0) hipCheck(cn_layer_set_dropout(m_handle, m_dropout), m_ctx);
    if (weightsSection && weightsSection->hasMember(name())) {                                                    // :68-101
        const json::Value &w = (*weightsSection)[name()];
        if (!w.isObject()) throw std::runtime_error("Weights section for layer '" + name() + "' is not an object");
        static const char *keys[3] = {"input", "bias", "internal"};
        for (int k = 0; k < 3; ++k)
            if (!w.hasMember(keys[k]) || !w[keys[k]].isArray())
                throw std::runtime_error("Missing array 'weights/" + name() + "/" + keys[k] + "'");
        const size_t P = (size_t)m_precedingLayer.size();
        if (w["input"].size() != (size_t)size() * inputWeightsPerBlock * P) throw std::runtime_error("Invalid number of input weights for layer '" + name() + "'");
        if (w["bias"].size() != (size_t)size() * inputWeightsPerBlock) throw std::runtime_error("Invalid number of bias weights for layer '" + name() + "'");
        if (w["internal"].size() != (size_t)size() * internalWeightsPerBlock) throw std::runtime_error("Invalid number of internal weights for layer '" + name() + "'");
        Hip::real_vector flat;
        flat.reserve(w["input"].size() + w["bias"].size() + w["internal"].size());
        for (int k = 0; k < 3; ++k)
            for (size_t i = 0; i < w[keys[k]].size(); ++i) flat.push_back((real_t)w[keys[k]][i].getDouble());
        setWeights(flat);
    }
    // otherwise NeuralNetwork draws the initial weights (TrainableLayer.cu:103-126)
}
int TrainableLayer::weightCount() const { return cn_layer_weight_count(m_handle); }
Hip::real_vector TrainableLayer::weights() const { return read(CN_BUF_WEIGHTS, 0, (size_t)weightCount()); }
Hip::real_vector TrainableLayer::weightUpdates() const { return read(CN_BUF_WEIGHT_UPDATES, 0, (size_t)weightCount()); }
void TrainableLayer::setWeights(const Hip::real_vector &w) { hipCheck(cn_layer_set_weights(m_handle, w.data(), (int)w.size()), m_ctx); }

void TrainableLayer::exportWeights(json::Value *weightsObject) const
{
    if (!weightsObject->isObject()) throw std::runtime_error("The JSON value is not an object");
    const Hip::real_vector w = weights();
    if (w.empty()) return;
    const size_t nIn = (size_t)size() * m_inputWeightsPerBlock * m_precedingLayer.size();
    const size_t nBias = (size_t)size() * m_inputWeightsPerBlock;
    json::Value in(json::Value::Array), bi(json::Value::Array), it(json::Value::Array);
    in.reserve(nIn); bi.reserve(nBias); it.reserve(w.size() - nIn - nBias);
    for (size_t i = 0; i < nIn; ++i) in.pushBack((double)w[i]);
    for (size_t i = 0; i < nBias; ++i) bi.pushBack((double)w[nIn + i]);
    for (size_t i = nIn + nBias; i < w.size(); ++i) it.pushBack((double)w[i]);
    json::Value sec(json::Value::Object);
    sec.addMember("input", in); sec.addMember("bias", bi); sec.addMember("internal", it);
    weightsObject->addMember(name(), sec);
}
void TrainableLayer::exportLayer(json::Value *layersArray) const
{
    Layer::exportLayer(layersArray);
    (*layersArray)[layersArray->size() - 1].addMember("bias", (double)m_bias);
    if (m_dropout > 0) (*layersArray)[layersArray->size() - 1].addMember("dropout", (double)m_dropout);
    if (residual()) (*layersArray)[layersArray->size() - 1].addMember("residual", true);
    if (layerNorm()) {
        (*layersArray)[layersArray->size() - 1].addMember("layer_norm", true);
        (*layersArray)[layersArray->size() - 1].addMember("layer_norm_eps", (double)layerNormEps());
    }
}

// ---- FeedForward / Softmax / Lstm -----------------------------------------------------------
FeedForwardLayer::FeedForwardLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer, cn_layer_kind kind)
    : TrainableLayer(ctx, layerChild, weightsSection, kind, 1, 0, precedingLayer)
    , m_type(kind == CN_LAYER_FF_TANH ? "feedforward_tanh" : (kind == CN_LAYER_FF_LOGISTIC ? "feedforward_logistic" : "feedforward_identity")) {}
const std::string &FeedForwardLayer::type() const { return m_type; }

SoftmaxLayer::SoftmaxLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer)
    : TrainableLayer(ctx, layerChild, weightsSection, CN_LAYER_SOFTMAX, 1, 0, precedingLayer) {}
const std::string &SoftmaxLayer::type() const { static const std::string s("softmax"); return s; }

LstmLayer::LstmLayer(cn_ctx *ctx, const json::Value &layerChild, const json::Value *weightsSection, Layer &precedingLayer, bool bidirectional)
    : TrainableLayer(ctx, layerChild, weightsSection, bidirectional ? CN_LAYER_BLSTM : CN_LAYER_LSTM, 4,
                     (bidirectional ? 2 : 4) * (layerChild.hasMember("size") ? layerChild["size"].getInt() : 0) + 3, precedingLayer)   // LstmLayer.cu:525
    , m_isBidirectional(bidirectional) {}
const std::string &LstmLayer::type() const
{
    static const std::string su("lstm"), sb("blstm");
    return m_isBidirectional ? sb : su;
}
Hip::real_vector LstmLayer::internal(cn_buffer which, int dir) const
{
    const int H = size() / (m_isBidirectional ? 2 : 1);
    return read(which, dir, (size_t)curMaxSeqLength() * parallelSequences() * H);
}

// ---- post output layers ---------------------------------------------------------------------
PostOutputLayer::PostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, cn_layer_kind kind, Layer &precedingLayer)
    : Layer(ctx, layerChild, kind, &precedingLayer, precedingLayer.parallelSequences(), precedingLayer.maxSeqLength(), 0.f)
    , m_precedingLayer(precedingLayer) {}
void PostOutputLayer::loadSequences(const data_sets::DataSetFraction &fraction)
{
    if (fraction.outputPatternSize() != size())                                                  // PostOutputLayer.cpp:70-73
        throw std::runtime_error("Output layer size of " + std::to_string(size()) + " != data target pattern size of " +
                                 std::to_string(fraction.outputPatternSize()));
    Layer::loadSequences(fraction);
}
real_t PostOutputLayer::calculateError()
{
    float e = 0; int c = 0;
    hipCheck(cn_loss_eval(m_handle, &e, &c), m_ctx);
    return e;
}

SsePostOutputLayer::SsePostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer)
    : PostOutputLayer(ctx, layerChild, CN_LAYER_SSE, precedingLayer) {}
const std::string &SsePostOutputLayer::type() const { static const std::string s("sse"); return s; }

MulticlassClassificationLayer::MulticlassClassificationLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer)
    : PostOutputLayer(ctx, layerChild, CN_LAYER_MULTICLASS_CLASSIFICATION, precedingLayer) {}
const std::string &MulticlassClassificationLayer::type() const { static const std::string s("multiclass_classification"); return s; }
int MulticlassClassificationLayer::countCorrectClassifications()
{
    float e = 0; int c = 0;
    hipCheck(cn_loss_eval(m_handle, &e, &c), m_ctx);
    return c;
}

CtcPostOutputLayer::CtcPostOutputLayer(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer)
    : PostOutputLayer(ctx, layerChild, CN_LAYER_CTC, precedingLayer) {}
const std::string &CtcPostOutputLayer::type() const { static const std::string s("ctc"); return s; }
void CtcPostOutputLayer::loadSequences(const data_sets::DataSetFraction &fraction)
{
    Layer::loadSequences(fraction);        // (labels are optional here: a forward pass over unlabelled data needs none)
}
void CtcPostOutputLayer::setLabelSequences(const data_sets::DataSetFraction &fraction)
{
    if ((int)fraction.labelSeqs().size() != fraction.numSequences()) return;    // no classification data: the error calls will say so
    std::vector<int> labels, lengths;
    for (size_t i = 0; i < fraction.labelSeqs().size(); ++i) {
        lengths.push_back((int)fraction.labelSeqs()[i].size());
        labels.insert(labels.end(), fraction.labelSeqs()[i].begin(), fraction.labelSeqs()[i].end());
    }
    hipCheck(cn_layer_set_label_sequences(m_handle, labels.data(), lengths.data(), (int)lengths.size()), m_ctx);
}
int CtcPostOutputLayer::countCorrectClassifications()
{
    float e = 0; int c = 0;
    hipCheck(cn_loss_eval(m_handle, &e, &c), m_ctx);
    return c;
}

#define CN_POST_LAYER(CLASS, KIND, TYPE)                                                                         \
    CLASS::CLASS(cn_ctx *ctx, const json::Value &layerChild, Layer &precedingLayer)                              \
        : PostOutputLayer(ctx, layerChild, KIND, precedingLayer) {}                                              \
    const std::string &CLASS::type() const { static const std::string s(TYPE); return s; }
CN_POST_LAYER(WeightedSsePostOutputLayer, CN_LAYER_WEIGHTEDSSE, "weightedsse")
CN_POST_LAYER(SseMaskPostOutputLayer, CN_LAYER_SSE_MASK, "wf")
CN_POST_LAYER(CePostOutputLayer, CN_LAYER_CE, "ce")
CN_POST_LAYER(RmsePostOutputLayer, CN_LAYER_RMSE, "rmse")
CN_POST_LAYER(BinaryClassificationLayer, CN_LAYER_BINARY_CLASSIFICATION, "binary_classification")
#undef CN_POST_LAYER
int BinaryClassificationLayer::countCorrectClassifications()
{
    float e = 0; int c = 0;
    hipCheck(cn_loss_eval(m_handle, &e, &c), m_ctx);
    return c;
}

}  // namespace layers
}  // namespace currennt_hip
