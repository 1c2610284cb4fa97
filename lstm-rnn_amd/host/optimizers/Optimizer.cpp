#include "Optimizer.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace currennt_hip {
namespace optimizers {

Optimizer::Optimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                     data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                     bool hybridOnlineBatch)
    : m_neuralNetwork(neuralNetwork), m_trainingSet(trainingSet), m_validationSet(validationSet), m_testSet(testSet)
    , m_maxEpochs(maxEpochs), m_maxEpochsNoBest(maxEpochsNoBest), m_validateEvery(validateEvery), m_testEvery(testEvery)
    , m_hybridOnlineBatch(hybridOnlineBatch)
    , m_finished(false), m_curEpoch(0), m_epochsSinceLowestError(0)
    , m_lowestValidationError(std::numeric_limits<real_t>::max()), m_curTrainingError(std::numeric_limits<real_t>::max())
    , m_curValidationError(std::numeric_limits<real_t>::max()), m_curTestError(std::numeric_limits<real_t>::max())
    , m_curValidationClassError(0), m_curTrainingClassError(0), m_curTestClassError(0)
{
    m_neuralNetwork.setExchangePerFraction(hybridOnlineBatch);
    m_bestWeights.resize(m_neuralNetwork.layers().size());
    _storeWeights();
}

void Optimizer::_storeWeights()
{
    const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) m_bestWeights[i] = layer->weights();
    }
}
void Optimizer::_restoreWeights()
{
    const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) layer->setWeights(m_bestWeights[i]);
    }
}

real_t Optimizer::_processDataSet(data_sets::DataSet &ds, bool calcWeightUpdates, real_t *classError)
{
    real_t error = 0;
    // the frames the output layer classifies: --input_frame_skip, and the strides of the context layers in front of it
    const int outRate = m_neuralNetwork.outputLayer().rate();
    const int classified = ds.totalNetworkTimesteps(outRate);
    *classError = (real_t)classified;
    const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
    const bool classification = dynamic_cast<layers::MulticlassClassificationLayer *>(&m_neuralNetwork.postOutputLayer()) != 0 ||
                                dynamic_cast<layers::BinaryClassificationLayer *>(&m_neuralNetwork.postOutputLayer()) != 0;   // Optimizer.cu:52-55

    // The reference reads the error of every fraction back (calculateError + countCorrectClassifications,
    // Optimizer.cu:46-55), which synchronises host and device once per fraction.  Here the per-fraction terms are
    // added up on the device, in the same order and in float like the reference's `error += ...`, and read back once
    // per pass over the data set: the host keeps enqueueing fractions while the device works.
    hipCheck(cn_loss_read(m_neuralNetwork.context(), nullptr, nullptr, 1), m_neuralNetwork.context());     // clear the sums
    // ctc: the class error of an evaluation pass is the LABEL ERROR RATE of best-path decoding, counted on the device beside the error
    // (include/currennt_hip.h, section CTC decoding) and read once per pass like it; of a training pass only with
    // --ctc_train_label_errors, else its class error stays unset.  Data-parallel: of this rank's sequences.
    const bool ctc = dynamic_cast<layers::CtcPostOutputLayer *>(&m_neuralNetwork.postOutputLayer()) != 0;
    const bool ctcDecode = ctc && (!calcWeightUpdates || m_ctcTrainLabelErrors);
    if (ctcDecode) hipCheck(cn_ctc_decode_read(m_neuralNetwork.context(), nullptr, nullptr, 1), m_neuralNetwork.context());     // clear the sums
    // dropout: only training passes drop; the calls are skipped altogether when no layer has a rate
    bool anyDropout = false;
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        const layers::TrainableLayer *layer = dynamic_cast<const layers::TrainableLayer *>(ls[i].get());
        anyDropout = anyDropout || (layer && layer->dropout() > 0);
    }
    if (anyDropout && !calcWeightUpdates) hipCheck(cn_ctx_set_dropout_pass(m_neuralNetwork.context(), 0, 0, 0), m_neuralNetwork.context());
    // input augmentation on the device: only training fractions; `index` is the fraction's index in the epoch
    auto setInputAugment = [&](uint64_t index) {
        cn_input_augment a = m_inputAugment;
        a.pass = ((uint64_t)m_curEpoch << 32) | (index & 0xFFFFFFFFull);
        hipCheck(cn_ctx_set_input_augment(m_neuralNetwork.context(), &a), m_neuralNetwork.context());
    };
    if (m_inputAugmentOn && !calcWeightUpdates) hipCheck(cn_ctx_set_input_augment(m_neuralNetwork.context(), nullptr), m_neuralNetwork.context());
    uint64_t fractionIndex = 0;
    data_sets::DataSetFraction frac, next;
    bool firstFraction = true;
    bool have = ds.getNextFraction(&frac);
    while (have) {
        if (anyDropout && calcWeightUpdates)
            hipCheck(cn_ctx_set_dropout_pass(m_neuralNetwork.context(), 1, m_dropoutSeed, ((uint64_t)m_curEpoch << 32) | (fractionIndex & 0xFFFFFFFFull)),
                     m_neuralNetwork.context());
        // weight noise generated on the device: the key of this fraction's backward pass (validation and test passes run none)
        const bool deviceNoise = calcWeightUpdates && m_weightNoiseOnDevice && m_weightNoiseSigma > 0;
        if (deviceNoise)
            hipCheck(cn_ctx_set_weight_noise(m_neuralNetwork.context(), m_weightNoiseSigma, m_weightNoiseSeed,
                                             ((uint64_t)m_curEpoch << 32) | (fractionIndex & 0xFFFFFFFFull)), m_neuralNetwork.context());
        const bool hostNoise = m_weightNoiseSigma > 0 && !m_weightNoiseOnDevice;
        if (m_inputAugmentOn && calcWeightUpdates) setInputAugment(fractionIndex);      // (what its prefetch was announced under)
        ++fractionIndex;
        m_neuralNetwork.loadSequences(frac);
        m_neuralNetwork.computeForwardPass();
        hipCheck(cn_loss_accumulate(m_neuralNetwork.postOutputLayer().handle()), m_neuralNetwork.context());
        if (ctcDecode) hipCheck(cn_ctc_decode_accumulate(m_neuralNetwork.postOutputLayer().handle()), m_neuralNetwork.context());
        // The data set's worker has the next fraction ready one ahead (DataSet.cpp:202-240,632-668); in training it goes on
        // across PCIe and through the re-layout beside this fraction's backward pass (cn_fraction_prefetch), and the load at
        // the top of the next iteration only exchanges buffers.  (`next` keeps its vectors' storage when it becomes `frac`:
        // the hint is matched by address.)
        const bool haveNext = ds.getNextFraction(&next);
        if (haveNext && calcWeightUpdates) {
            if (m_inputAugmentOn) setInputAugment(fractionIndex);      // the next fraction's settings, in front of its announcement
            m_neuralNetwork.prefetchSequences(next);
        }

        if (calcWeightUpdates) {
            // weight noise: the forward pass above used the clean weights, the backward pass runs on noisy ones
            // and the clean weights come back before the update (Optimizer.cu:58-68, :82-84).  The noise is
            // drawn on the host like the reference's (TrainableLayer.cu:188-209), std::mt19937 instead of boost's -- unless
            // --weight_noise_on_device: then the library generates it into the copies the backward pass reads (set above),
            // nothing is uploaded or restored and the update may be armed.
            std::vector<Hip::real_vector> origWeights(ls.size());
            if (hostNoise) {
                std::normal_distribution<real_t> dist(0.0f, m_weightNoiseSigma);
                for (size_t i = 1; i + 1 < ls.size(); ++i) {
                    layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
                    if (!layer) continue;
                    origWeights[i] = layer->weights();
                    Hip::real_vector noisy = origWeights[i];
                    for (size_t k = 0; k < noisy.size(); ++k) noisy[k] += dist(m_noiseGen);
                    layer->setWeights(noisy);
                }
            }
            if (m_hybridOnlineBatch && !hostNoise) { _setScheduledLayerRates(); _armUpdate(); }
            m_neuralNetwork.computeBackwardPass();
            if (hostNoise) {
                hipCheck(cn_ctx_join(m_neuralNetwork.context()), m_neuralNetwork.context());   // gradient GEMMs still read the noisy operands
                for (size_t i = 1; i + 1 < ls.size(); ++i) {
                    layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
                    if (layer) layer->setWeights(origWeights[i]);
                }
            }
            if (m_hybridOnlineBatch) {
                _completeUpdate();                                          // Optimizer.cu:88-89
            } else {
                // batch learning: sum the fractions' weightUpdates, one update per epoch (:72-85, :95-97) -- on the device,
                // one launch over all layers, like the reference's thrust::copy / thrust::transform(plus)
                hipCheck(cn_ctx_accumulate_updates(m_neuralNetwork.context(), firstFraction ? 1 : 0), m_neuralNetwork.context());
            }
        }
        firstFraction = false;
        have = haveNext;
        if (have) std::swap(frac, next);
    }
    if (calcWeightUpdates && !m_hybridOnlineBatch) _completeUpdate();
    {
        float e = 0; int64_t correct = 0;
        // data-parallel: the sums of all ranks (every rank then computes the same epoch errors and takes the same
        // early-stopping decisions)
        if (m_neuralNetwork.dataParallel())
            hipCheck(cn_loss_read_global(m_neuralNetwork.context(), &e, &correct, 1), m_neuralNetwork.context());
        else
            hipCheck(cn_loss_read(m_neuralNetwork.context(), &e, &correct, 1), m_neuralNetwork.context());
        error = e;
        if (classification) *classError -= (real_t)correct;
    }
    error /= ds.totalSequences();                                           // :99-101
    *classError /= (real_t)classified;
    if (ctcDecode) {
        int64_t labelErrors = 0, labelCount = 0;
        hipCheck(cn_ctc_decode_read(m_neuralNetwork.context(), &labelErrors, &labelCount, 1), m_neuralNetwork.context());
        *classError = labelCount ? (real_t)labelErrors / (real_t)labelCount : 0;
    } else if (ctc) *classError = 0;
    return error;
}

// One epoch (Optimizer.cu:283-324): train, then -- on the epochs the options ask for -- score the validation and test sets,
// keep the weights of the best validation epoch, and decide whether to stop.  Split into the three questions an epoch asks.
bool Optimizer::train()
{
    if (m_finished) return true;
    ++m_curEpoch;
    m_curTrainingError = _processDataSet(m_trainingSet, true, &m_curTrainingClassError);
    // weight averaging: the evaluation passes and the best weights kept (_storeWeights, an empty validation set included) see the
    // average; the raw weights are back before the stop decision, whose _restoreWeights() writes them
    const bool swapped = swapWeightAverage();
    _scoreValidationSet();
    if (_dueThisEpoch(m_testSet, m_testEvery)) m_curTestError = _processDataSet(m_testSet, false, &m_curTestClassError);
    if (swapped) swapWeightAverage();
    // learning-rate schedule: the epoch's monitored error, beside early stopping (which is untouched)
    if (m_schedule.on()) {
        if (m_validationSet.empty()) m_schedule.epochEnd((double)m_curTrainingError);
        else if (_dueThisEpoch(m_validationSet, m_validateEvery)) m_schedule.epochEnd((double)m_curValidationError);
    }
    if (_shouldStop()) {
        _restoreWeights();          // training ends on the best weights seen, not on the last ones
        m_finished = true;
    }
    return m_finished;
}

// the update of the optimizer at hand, then the averaging step it completes (hybrid online/batch and batch learning, host or
// device noise: every path to an update comes through here)
void Optimizer::_completeUpdate()
{
    _setScheduledLayerRates();          // (the values the arming call named, if one came: the count below is what moves them)
    _updateWeights();
    m_schedule.countUpdate();
    if (!(m_avgDecay > 0)) return;
    const int64_t k = ++m_avgSteps;
    double decay = (double)m_avgDecay;
    if (m_avgWarmup && k >= 2) decay = std::min(decay, (double)k / ((double)k + 9.0));
    hipCheck(cn_ctx_average_weights(m_neuralNetwork.context(), (float)decay), m_neuralNetwork.context());
}

void Optimizer::_setScheduledLayerRates()
{
    if (!m_schedule.on()) return;
    const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer && layer->learningRate() >= 0.0)
            hipCheck(cn_layer_set_learning_rate(layer->handle(), m_schedule.scaled(layer->learningRate())), m_neuralNetwork.context());
    }
}

bool Optimizer::swapWeightAverage()
{
    if (!(m_avgDecay > 0)) return false;
    int exists = 0;
    hipCheck(cn_ctx_weight_average_state(m_neuralNetwork.context(), &exists, nullptr), m_neuralNetwork.context());
    if (!exists) return false;          // (no update yet: nothing to exchange)
    hipCheck(cn_ctx_swap_weight_average(m_neuralNetwork.context()), m_neuralNetwork.context());
    return true;
}

bool Optimizer::_dueThisEpoch(const data_sets::DataSet &set, int every) const
{
    return !set.empty() && m_curEpoch % every == 0;
}

void Optimizer::_scoreValidationSet()
{
    if (m_validationSet.empty()) {
        // nothing to select on: every epoch counts as the best so far
        m_epochsSinceLowestError = 0;
        _storeWeights();
        return;
    }
    if (!_dueThisEpoch(m_validationSet, m_validateEvery)) return;
    m_curValidationError = _processDataSet(m_validationSet, false, &m_curValidationClassError);
    const bool improved = m_curValidationError < m_lowestValidationError;
    if (improved) {
        m_lowestValidationError = m_curValidationError;
        m_epochsSinceLowestError = 0;
        _storeWeights();
    } else {
        m_epochsSinceLowestError += m_validateEvery;
    }
}

bool Optimizer::_shouldStop() const
{
    const bool noProgress = m_epochsSinceLowestError >= m_maxEpochsNoBest;
    const bool outOfEpochs = m_maxEpochs >= 0 && m_curEpoch >= m_maxEpochs;
    return noProgress || outOfEpochs;
}

void Optimizer::_exportWeights(json::Value *jsonDoc, const char *arrayName, const std::vector<Hip::real_vector> &weights)
{
    json::Value weightsArray(json::Value::Array);
    for (size_t i = 0; i < weights.size(); ++i) {
        json::Value v(json::Value::Array);
        v.reserve(weights[i].size());
        for (size_t j = 0; j < weights[i].size(); ++j) v.pushBack(json::Value((double)weights[i][j]));
        weightsArray.pushBack(v);
    }
    jsonDoc->addMember(arrayName, weightsArray);
}
void Optimizer::_importWeights(const json::Value &jsonDoc, const char *arrayName, std::vector<Hip::real_vector> *weights)
{
    if (!jsonDoc.hasMember(arrayName) || !jsonDoc[arrayName].isArray())
        throw std::runtime_error(std::string("Array '") + arrayName + "' is missing or has the wrong type");
    const json::Value &arr = jsonDoc[arrayName];
    if (arr.size() != weights->size()) throw std::runtime_error(std::string("Array '") + arrayName + "' has a wrong size");
    for (size_t i = 0; i < arr.size(); ++i) {
        if (!arr[i].isArray()) throw std::runtime_error(std::string("Object in '") + arrayName + "' is not an array");
        if (arr[i].size() != (*weights)[i].size()) throw std::runtime_error(std::string("Subarray in '") + arrayName + "' has a wrong size");
        for (size_t j = 0; j < arr[i].size(); ++j) (*weights)[i][j] = (real_t)arr[i][j].getDouble();
    }
}

// Autosave state (Optimizer.cu:326-358; the JSON keys are the reference's file format).  One table names every scalar of
// the state once; export and import both walk it.
namespace {
struct IntField  { const char *key; int Optimizer::*member; };
struct RealField { const char *key; real_t Optimizer::*member; };
}  // namespace

struct Optimizer::StateTable {
    static const std::vector<IntField> &ints()
    {
        static const std::vector<IntField> t = {
            {"optimizer_cur_epoch", &Optimizer::m_curEpoch},
            {"optimizer_epochs_since_lowest_error", &Optimizer::m_epochsSinceLowestError},
        };
        return t;
    }
    static const std::vector<RealField> &reals()
    {
        static const std::vector<RealField> t = {
            {"optimizer_lowest_validation_error", &Optimizer::m_lowestValidationError},
            {"optimizer_cur_training_error", &Optimizer::m_curTrainingError},
            {"optimizer_cur_validation_error", &Optimizer::m_curValidationError},
            {"optimizer_cur_test_error", &Optimizer::m_curTestError},
            {"optimizer_cur_training_class_error", &Optimizer::m_curTrainingClassError},
            {"optimizer_cur_validation_class_error", &Optimizer::m_curValidationClassError},
            {"optimizer_cur_test_class_error", &Optimizer::m_curTestClassError},
        };
        return t;
    }
};

void Optimizer::exportState(json::Value *jsonDoc) const
{
    jsonDoc->addMember("optimizer_finished", json::Value(m_finished));
    for (const IntField &f : StateTable::ints()) jsonDoc->addMember(f.key, json::Value(this->*f.member));
    for (const RealField &f : StateTable::reals()) jsonDoc->addMember(f.key, json::Value((double)(this->*f.member)));
    _exportWeights(jsonDoc, "optimizer_best_weights", m_bestWeights);
    // learning-rate schedule: its four state members (the two doubles as text with 17 digits: the file's numbers keep 9)
    if (m_schedule.on()) {
        const LearningRateSchedule::State &st = m_schedule.state();
        char scale[40], lowest[40];
        snprintf(scale, sizeof(scale), "%.17g", st.scale); snprintf(lowest, sizeof(lowest), "%.17g", st.lowest);
        jsonDoc->addMember("optimizer_updates", json::Value((double)st.updates));
        jsonDoc->addMember("learning_rate_scale", json::Value(std::string(scale)));
        jsonDoc->addMember("learning_rate_bad_epochs", json::Value(st.bad));
        jsonDoc->addMember("learning_rate_lowest_error", json::Value(std::string(lowest)));
    }
    // weight averaging: the average (laid out like optimizer_best_weights) and the number of averaging steps taken
    if (m_avgDecay > 0) {
        const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
        std::vector<Hip::real_vector> avg(ls.size());
        for (size_t i = 1; i + 1 < ls.size(); ++i) {
            layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
            if (!layer) continue;
            avg[i].resize(layer->weightCount());
            hipCheck(cn_layer_read_weight_average(layer->handle(), avg[i].data(), avg[i].size()), m_neuralNetwork.context());
        }
        _exportWeights(jsonDoc, "weight_average", avg);
        jsonDoc->addMember("weight_average_steps", json::Value((double)m_avgSteps));
    }
}
void Optimizer::importState(const json::Value &jsonDoc)
{
    m_finished = jsonDoc["optimizer_finished"].getBool();
    for (const IntField &f : StateTable::ints()) this->*f.member = jsonDoc[f.key].getInt();
    for (const RealField &f : StateTable::reals()) this->*f.member = (real_t)jsonDoc[f.key].getDouble();
    _importWeights(jsonDoc, "optimizer_best_weights", &m_bestWeights);
    // learning-rate schedule on, and the file has no state of it (it was written without a schedule): the schedule starts fresh
    if (m_schedule.on()) {
        if (jsonDoc.hasMember("optimizer_updates") && jsonDoc.hasMember("learning_rate_scale") && jsonDoc.hasMember("learning_rate_bad_epochs") &&
            jsonDoc.hasMember("learning_rate_lowest_error")) {
            LearningRateSchedule::State st;
            st.updates = (int64_t)jsonDoc["optimizer_updates"].getDouble();
            st.scale = strtod(jsonDoc["learning_rate_scale"].getString().c_str(), nullptr);
            st.bad = jsonDoc["learning_rate_bad_epochs"].getInt();
            st.lowest = strtod(jsonDoc["learning_rate_lowest_error"].getString().c_str(), nullptr);
            m_schedule.setState(st);
        } else m_scheduleStartsFresh = true;
    }
    // weight averaging off: an average in the file is ignored.  On, and the file has none (it was written without averaging): the
    // average starts fresh at the next update
    if (!(m_avgDecay > 0)) return;
    if (!jsonDoc.hasMember("weight_average")) {
        m_avgStartsFresh = true;
        m_avgSteps = 0;
        return;
    }
    const std::vector<std::shared_ptr<layers::Layer> > &ls = m_neuralNetwork.layers();
    std::vector<Hip::real_vector> avg(ls.size());
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) avg[i].resize(layer->weightCount());
    }
    _importWeights(jsonDoc, "weight_average", &avg);
    m_avgSteps = jsonDoc.hasMember("weight_average_steps") ? (int64_t)jsonDoc["weight_average_steps"].getDouble() : 0;
    if (m_avgSteps < 1) return;         // (written before the first update: the first step copies, as it would have)
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) hipCheck(cn_layer_upload_weight_average(layer->handle(), avg[i].data(), avg[i].size()), m_neuralNetwork.context());
    }
}

// the momentum state lives on the device (CN_BUF_WEIGHT_DELTAS); autosave moves it through the host
void SteepestDescentOptimizer::exportState(json::Value *jsonDoc) const
{
    Optimizer::exportState(jsonDoc);
    NeuralNetwork &nn = const_cast<SteepestDescentOptimizer *>(this)->_neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    std::vector<Hip::real_vector> deltas(ls.size());
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        deltas[i].resize(layer->weightCount());
        hipCheck(cn_layer_read(layer->handle(), CN_BUF_WEIGHT_DELTAS, 0, deltas[i].data(), deltas[i].size()), nn.context());
    }
    _exportWeights(jsonDoc, "steepest_descent_optimizer_weight_deltas", deltas);
}
void SteepestDescentOptimizer::importState(const json::Value &jsonDoc)
{
    if (jsonDoc.hasMember("lamb_optimizer"))
        throw std::runtime_error("The autosave file was written by the lamb optimizer and cannot be continued with steepest_descent");
    if (jsonDoc.hasMember("adam_optimizer_step"))
        throw std::runtime_error("The autosave file was written by the adam optimizer and cannot be continued with steepest_descent");
    Optimizer::importState(jsonDoc);
    NeuralNetwork &nn = _neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    std::vector<Hip::real_vector> deltas(ls.size());
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) deltas[i].resize(layer->weightCount());
    }
    _importWeights(jsonDoc, "steepest_descent_optimizer_weight_deltas", &deltas);
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) hipCheck(cn_layer_upload(layer->handle(), CN_BUF_WEIGHT_DELTAS, deltas[i].data(), deltas[i].size()), nn.context());
    }
}

SteepestDescentOptimizer::SteepestDescentOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet,
                                                   data_sets::DataSet &validationSet, data_sets::DataSet &testSet, int maxEpochs,
                                                   int maxEpochsNoBest, int validateEvery, int testEvery, real_t learningRate,
                                                   real_t momentum, bool hybridOnlineBatch)
    : Optimizer(neuralNetwork, trainingSet, validationSet, testSet, maxEpochs, maxEpochsNoBest, validateEvery, testEvery, hybridOnlineBatch)
    , m_learningRate(learningRate), m_momentum(momentum) {}

void SteepestDescentOptimizer::_armUpdate()
{
    NeuralNetwork &nn = _neuralNetwork();
    hipCheck(cn_ctx_arm_update(nn.context(), _scheduledRate(m_learningRate), m_momentum), nn.context());
}

void SteepestDescentOptimizer::_updateWeights()
{
    NeuralNetwork &nn = _neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    if (!hybridOnlineBatch()) {
        // batch mode: the epoch sum becomes the weightUpdates again before the update (device to device); data-parallel ranks
        // then add their epoch sums up in one exchange over the whole arena
        hipCheck(cn_ctx_take_accumulated(nn.context()), nn.context());
        if (nn.dataParallel()) hipCheck(cn_allreduce_grads(nn.context(), 0, 0), nn.context());
    }
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        real_t lr = m_learningRate;
        if (layer->learningRate() >= 0.0) lr = layer->learningRate();        // SteepestDescentOptimizer.cu:78-80
        lr = _scheduledRate(lr);
        hipCheck(cn_sgd_update(layer->handle(), lr, m_momentum), nn.context());
    }
}

void Optimizer::setWeightDecay(real_t decay)
{
    hipCheck(cn_ctx_set_weight_decay(m_neuralNetwork.context(), decay), m_neuralNetwork.context());
}

void Optimizer::setMaxGradNorm(real_t maxNorm)
{
    hipCheck(cn_ctx_set_grad_clip(m_neuralNetwork.context(), maxNorm), m_neuralNetwork.context());
}

Optimizer::ClipStats Optimizer::takeClipStats()
{
    ClipStats s{};
    int64_t updates = 0, clipped = 0, skipped = 0;
    hipCheck(cn_ctx_grad_clip_stats(m_neuralNetwork.context(), nullptr, nullptr, &updates, &clipped, &skipped, &s.maxNormSeen, 1), m_neuralNetwork.context());
    s.updates = updates; s.clipped = clipped; s.skipped = skipped;
    return s;
}

AdamOptimizer::AdamOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                             data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                             real_t learningRate, real_t beta1, real_t beta2, real_t epsilon, bool hybridOnlineBatch)
    : Optimizer(neuralNetwork, trainingSet, validationSet, testSet, maxEpochs, maxEpochsNoBest, validateEvery, testEvery, hybridOnlineBatch)
    , m_learningRate(learningRate), m_beta1(beta1), m_beta2(beta2), m_epsilon(epsilon), m_step(0), m_armed(false) {}

void AdamOptimizer::_armUpdate()
{
    NeuralNetwork &nn = _neuralNetwork();
    ++m_step;
    m_armed = true;
    hipCheck(_armCall(_scheduledRate(m_learningRate)), nn.context());
}
int AdamOptimizer::_armCall(real_t lr) { return cn_ctx_arm_adam(_neuralNetwork().context(), lr, m_beta1, m_beta2, m_epsilon, m_step); }
int AdamOptimizer::_layerCall(cn_layer *layer, real_t lr) { return cn_adam_update(layer, lr, m_beta1, m_beta2, m_epsilon, m_step); }

void AdamOptimizer::_updateWeights()
{
    NeuralNetwork &nn = _neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    if (!m_armed) ++m_step;
    m_armed = false;
    if (!hybridOnlineBatch()) {              // batch mode: as in SteepestDescentOptimizer::_updateWeights
        hipCheck(cn_ctx_take_accumulated(nn.context()), nn.context());
        if (nn.dataParallel()) hipCheck(cn_allreduce_grads(nn.context(), 0, 0), nn.context());
    }
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        real_t lr = m_learningRate;
        if (layer->learningRate() >= 0.0) lr = layer->learningRate();        // a layer's own "learningRate" is its Adam step size
        lr = _scheduledRate(lr);
        hipCheck(_layerCall(layer->handle(), lr), nn.context());
    }
}

// both moment vectors live on the device (CN_BUF_WEIGHT_DELTAS, CN_BUF_ADAM_SECOND_MOMENTS); autosave moves them through the host
void AdamOptimizer::exportState(json::Value *jsonDoc) const
{
    Optimizer::exportState(jsonDoc);
    NeuralNetwork &nn = const_cast<AdamOptimizer *>(this)->_neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    std::vector<Hip::real_vector> m(ls.size()), v(ls.size());
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        m[i].resize(layer->weightCount()); v[i].resize(layer->weightCount());
        hipCheck(cn_layer_read(layer->handle(), CN_BUF_WEIGHT_DELTAS, 0, m[i].data(), m[i].size()), nn.context());
        hipCheck(cn_layer_read(layer->handle(), CN_BUF_ADAM_SECOND_MOMENTS, 0, v[i].data(), v[i].size()), nn.context());
    }
    _exportWeights(jsonDoc, "adam_optimizer_first_moments", m);
    _exportWeights(jsonDoc, "adam_optimizer_second_moments", v);
    jsonDoc->addMember("adam_optimizer_step", json::Value((double)m_step));
}
void AdamOptimizer::importState(const json::Value &jsonDoc)
{
    if (!jsonDoc.hasMember("adam_optimizer_step")) {
        if (jsonDoc.hasMember("steepest_descent_optimizer_weight_deltas"))
            throw std::runtime_error(std::string("The autosave file was written by the steepest_descent optimizer and cannot be continued with ") + _name());
        throw std::runtime_error("Value 'adam_optimizer_step' is missing in the autosave file");
    }
    const bool lambFile = jsonDoc.hasMember("lamb_optimizer"), lamb = std::string(_name()) == "lamb";
    if (lambFile != lamb)
        throw std::runtime_error(std::string("The autosave file was written by the ") + (lambFile ? "lamb" : "adam") +
                                 " optimizer and cannot be continued with " + _name());
    Optimizer::importState(jsonDoc);
    NeuralNetwork &nn = _neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    std::vector<Hip::real_vector> m(ls.size()), v(ls.size());
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (layer) { m[i].resize(layer->weightCount()); v[i].resize(layer->weightCount()); }
    }
    _importWeights(jsonDoc, "adam_optimizer_first_moments", &m);
    _importWeights(jsonDoc, "adam_optimizer_second_moments", &v);
    m_step = (int64_t)jsonDoc["adam_optimizer_step"].getDouble();
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        hipCheck(cn_layer_upload(layer->handle(), CN_BUF_WEIGHT_DELTAS, m[i].data(), m[i].size()), nn.context());
        hipCheck(cn_layer_upload(layer->handle(), CN_BUF_ADAM_SECOND_MOMENTS, v[i].data(), v[i].size()), nn.context());
    }
}

LambOptimizer::LambOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                             data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                             real_t learningRate, real_t beta1, real_t beta2, real_t epsilon, real_t minTrust, real_t maxTrust, bool hybridOnlineBatch)
    : AdamOptimizer(neuralNetwork, trainingSet, validationSet, testSet, maxEpochs, maxEpochsNoBest, validateEvery, testEvery, learningRate,
                    beta1, beta2, epsilon, hybridOnlineBatch)
    , m_minTrust(minTrust), m_maxTrust(maxTrust)
{
    hipCheck(cn_ctx_set_trust_bounds(neuralNetwork.context(), m_minTrust, m_maxTrust), neuralNetwork.context());
}
int LambOptimizer::_armCall(real_t lr) { return cn_ctx_arm_lamb(_neuralNetwork().context(), lr, m_beta1, m_beta2, m_epsilon, m_step); }
int LambOptimizer::_layerCall(cn_layer *layer, real_t lr) { return cn_lamb_update(layer, lr, m_beta1, m_beta2, m_epsilon, m_step); }

void LambOptimizer::exportState(json::Value *jsonDoc) const
{
    AdamOptimizer::exportState(jsonDoc);
    jsonDoc->addMember("lamb_optimizer", json::Value(true));
    jsonDoc->addMember("lamb_optimizer_min_trust", json::Value((double)m_minTrust));
    jsonDoc->addMember("lamb_optimizer_max_trust", json::Value((double)m_maxTrust));
}
void LambOptimizer::importState(const json::Value &jsonDoc)
{
    AdamOptimizer::importState(jsonDoc);
    if (jsonDoc.hasMember("lamb_optimizer_min_trust")) m_minTrust = (real_t)jsonDoc["lamb_optimizer_min_trust"].getDouble();
    if (jsonDoc.hasMember("lamb_optimizer_max_trust")) m_maxTrust = (real_t)jsonDoc["lamb_optimizer_max_trust"].getDouble();
    NeuralNetwork &nn = _neuralNetwork();
    hipCheck(cn_ctx_set_trust_bounds(nn.context(), m_minTrust, m_maxTrust), nn.context());
}

LambOptimizer::TrustRange LambOptimizer::trustRange()
{
    NeuralNetwork &nn = _neuralNetwork();
    const std::vector<std::shared_ptr<layers::Layer> > &ls = nn.layers();
    TrustRange r{0.f, 0.f, "", ""};
    bool first = true;
    for (size_t i = 1; i + 1 < ls.size(); ++i) {
        layers::TrainableLayer *layer = dynamic_cast<layers::TrainableLayer *>(ls[i].get());
        if (!layer) continue;
        float ratio = 1.f;
        hipCheck(cn_layer_trust_ratio(layer->handle(), &ratio, nullptr, nullptr), nn.context());
        if (first || ratio < r.min) { r.min = ratio; r.minLayer = layer->name(); }
        if (first || ratio > r.max) { r.max = ratio; r.maxLayer = layer->name(); }
        first = false;
    }
    return r;
}

}  // namespace optimizers
}  // namespace currennt_hip
