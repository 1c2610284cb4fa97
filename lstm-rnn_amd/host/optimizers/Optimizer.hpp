// Epoch protocol and momentum SGD (currennt_lib/src/optimizers/{Optimizer,SteepestDescentOptimizer}.*), and Adam and LAMB beside it.
// Gradient accumulation, the update and best-weight bookkeeping all stay on the device; the host only
// sequences them.
#pragma once

#include <random>
#include <vector>

#include "../Json.hpp"
#include "../NeuralNetwork.hpp"
#include "../data_sets/DataSet.hpp"
#include "LearningRateSchedule.hpp"

namespace currennt_hip {
namespace optimizers {

class Optimizer {
public:
    Optimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
              data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
              bool hybridOnlineBatch);
    virtual ~Optimizer() {}

    // Gaussian weight noise during the backward pass (Optimizer.cu:58-68,82-84; --weight_noise_sigma)
    void setWeightNoise(real_t sigma, unsigned randomSeed) { m_weightNoiseSigma = sigma; m_noiseGen.seed(randomSeed); }
    // --weight_noise_on_device (include/currennt_hip.h, section Weight noise): the same sigma, generated on the device with this
    // seed -- the same on every rank, so the replicas perturb the same weights the same way -- and pass = (epoch << 32) | index of
    // the fraction in the epoch: derived, not stored, so --continue resumes the same noise.  No host copies, no join, and the
    // update of hybrid online/batch learning stays armed.
    void setWeightNoiseOnDevice(bool onDevice, uint64_t seed) { m_weightNoiseOnDevice = onDevice; m_weightNoiseSeed = seed; }
    // --input_noise_on_device / --spec_augment_* (include/currennt_hip.h, section Input augmentation): the training fractions are
    // re-laid out with these settings -- seed as for dropout (each rank holds other sequences), pass = (epoch << 32) | index of the
    // fraction in the epoch, derived like dropout's -- set in front of each fraction's prefetch announcement and again in front
    // of its load, so the load stays a hit; validation and test passes load without augmentation
    void setInputAugment(const cn_input_augment &settings) { m_inputAugment = settings; m_inputAugmentOn = true; }
    // ctc nets (--ctc_train_label_errors): training passes count label errors too, on the posteriors their own forward pass produced
    // (include/currennt_hip.h, section CTC decoding); curTrainingClassError() is then the training pass's label error rate
    void setCtcTrainLabelErrors(bool on) { m_ctcTrainLabelErrors = on; }
    // Dropout (layers with a JSON "dropout"; include/currennt_hip.h, section Dropout): training passes drop with this seed and
    // pass = (epoch << 32) | index of the fraction in the epoch -- derived, not stored, so --continue resumes the same masks;
    // validation and test passes do not drop
    void setDropoutSeed(uint64_t seed) { m_dropoutSeed = seed; }
    // --max_grad_norm (include/currennt_hip.h, section Gradient clipping): the bound is set once, 0 = off; the device keeps the
    // statistics, takeClipStats reads and resets them (one synchronising call, once per epoch)
    void setMaxGradNorm(real_t maxNorm);
    struct ClipStats { float maxNormSeen; long long updates, clipped, skipped; };
    ClipStats takeClipStats();
    // --weight_decay (include/currennt_hip.h, section Weight decay): set once on the context, 0 = off; every update of either
    // optimizer and either learning mode then decays the input and recurrent weights by lr * decay of themselves
    void setWeightDecay(real_t decay);
    // --learning_rate_warmup_updates / --learning_rate_decay / --learning_rate_decay_patience / --learning_rate_min
    // (LearningRateSchedule.hpp): every update runs at the schedule's factor -- the global rate and a layer's own "learningRate"
    // alike, the armed call and the completing call of one step at the same value -- and every epoch that has a monitored error
    // (the validation error where one was computed, the average's under weight averaging; the training error without a
    // validation set) reports it to the schedule.  The state travels with the autosave.  A schedule that is off changes nothing.
    void setLearningRateSchedule(const LearningRateSchedule &schedule) { m_schedule = schedule; }
    const LearningRateSchedule &learningRateSchedule() const { return m_schedule; }
    // importState found no schedule state in the autosave file although the schedule is on: it starts fresh
    bool learningRateScheduleStartsFresh() const { return m_scheduleStartsFresh; }
    // --weight_average_decay / --weight_average_warmup (include/currennt_hip.h, section Weight averaging): one averaging step behind
    // every completed update, whichever optimizer and learning mode; step k (from 1, kept here: the library keeps no clock, and it
    // travels with the autosave) uses `decay`, with warm-up min(decay, k / (k + 9)) for k >= 2.  Between an epoch's training pass
    // and its stop decision the weights and the average are exchanged: the validation and test errors, early stopping and the
    // best weights kept -- and so trained_network.jsn -- are the average's.  decay 0 = off.
    void setWeightAverage(real_t decay, bool warmup) { m_avgDecay = decay; m_avgWarmup = warmup; }
    // Exchanges the weights and the average if averaging is on and an average exists (returns whether it did): the driver saves
    // the .best.jsn network between two calls
    bool swapWeightAverage();
    // importState found no average in the autosave file although averaging is on (it was written without): it starts fresh
    bool weightAverageStartsFresh() const { return m_avgStartsFresh; }
    // autosave / --continue (Optimizer.cu:326-358)
    virtual void exportState(json::Value *jsonDoc) const;
    virtual void importState(const json::Value &jsonDoc);

    bool finished() const { return m_finished; }
    int currentEpoch() const { return m_curEpoch; }
    real_t lowestValidationError() const { return m_lowestValidationError; }
    int epochsSinceLowestValidationError() const { return m_epochsSinceLowestError; }
    real_t curTrainingError() const { return m_curTrainingError; }
    real_t curValidationError() const { return m_curValidationError; }
    real_t curTestError() const { return m_curTestError; }
    real_t curTrainingClassError() const { return m_curTrainingClassError; }
    real_t curValidationClassError() const { return m_curValidationClassError; }
    real_t curTestClassError() const { return m_curTestClassError; }

    bool train();                                                       // Optimizer.cu:283-324

protected:
    virtual void _updateWeights() = 0;
    // hybrid online/batch learning without weight noise drawn on the host: the update of the coming backward pass may be applied layer by layer
    // behind each layer's gradient (cn_ctx_arm_update); _updateWeights() then only completes it
    virtual void _armUpdate() {}
    real_t _processDataSet(data_sets::DataSet &ds, bool calcWeightUpdates, real_t *classError);   // Optimizer.cu:37-104
    void _scoreValidationSet();                                         // validation part of train()
    bool _dueThisEpoch(const data_sets::DataSet &set, int every) const;
    bool _shouldStop() const;
    struct StateTable;                                                  // scalars of the autosave state (Optimizer.cpp)
    void _storeWeights();                                               // :151-158
    void _restoreWeights();                                             // :160-168
    NeuralNetwork &_neuralNetwork() { return m_neuralNetwork; }
    // `rate` as the update about to be armed or made uses it (the schedule's factor; `rate` itself with the schedule off)
    real_t _scheduledRate(real_t rate) const { return m_schedule.on() ? m_schedule.scaled(rate) : rate; }
    // (the reference's `_curWeightUpdates()`, the epoch sum of batch learning, lives on the device: cn_ctx_accumulate_updates /
    // cn_ctx_take_accumulated)

private:
    NeuralNetwork &m_neuralNetwork;
    data_sets::DataSet &m_trainingSet, &m_validationSet, &m_testSet;
    const int m_maxEpochs, m_maxEpochsNoBest, m_validateEvery, m_testEvery;
    const bool m_hybridOnlineBatch;
    bool m_finished;
    int m_curEpoch, m_epochsSinceLowestError;
    real_t m_lowestValidationError, m_curTrainingError, m_curValidationError, m_curTestError,
           m_curValidationClassError, m_curTrainingClassError, m_curTestClassError;
    std::vector<Hip::real_vector> m_bestWeights;
    real_t m_weightNoiseSigma = 0;
    std::mt19937 m_noiseGen;
    bool m_weightNoiseOnDevice = false;
    uint64_t m_weightNoiseSeed = 0;
    uint64_t m_dropoutSeed = 0;
    cn_input_augment m_inputAugment{};
    bool m_inputAugmentOn = false;
    bool m_ctcTrainLabelErrors = false;
    real_t m_avgDecay = 0;
    bool m_avgWarmup = true, m_avgStartsFresh = false;
    int64_t m_avgSteps = 0;             // averaging steps taken so far
    void _completeUpdate();             // _updateWeights(), then the averaging step
    LearningRateSchedule m_schedule;
    bool m_scheduleStartsFresh = false;
    void _setScheduledLayerRates();     // schedule on: the layers' own rates at the factor of the update about to be armed or made
protected:
    static void _exportWeights(json::Value *jsonDoc, const char *arrayName, const std::vector<Hip::real_vector> &weights);   // :106-123
    static void _importWeights(const json::Value &jsonDoc, const char *arrayName, std::vector<Hip::real_vector> *weights);   // :125-149
    bool hybridOnlineBatch() const { return m_hybridOnlineBatch; }
};

class SteepestDescentOptimizer : public Optimizer {
public:
    SteepestDescentOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                             data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                             real_t learningRate, real_t momentum, bool hybridOnlineBatch);
    void exportState(json::Value *jsonDoc) const;                       // SteepestDescentOptimizer.cu:118-131
    void importState(const json::Value &jsonDoc);
protected:
    void _updateWeights();                                              // SteepestDescentOptimizer.cu:67-94
    void _armUpdate();
private:
    real_t m_learningRate, m_momentum;
};

// Adam (include/currennt_hip.h, cn_adam_update; the reference has no counterpart: its second optimizer is rprop,
// Configuration.cpp:152,265).  Stands beside SteepestDescentOptimizer on the same two seams, so hybrid online/batch and batch
// learning, weight noise and --gpus N sequence it exactly as they sequence steepest descent.  The library keeps no clock: the
// update count lives here and travels with the autosave.
class AdamOptimizer : public Optimizer {
public:
    AdamOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                  data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                  real_t learningRate, real_t beta1, real_t beta2, real_t epsilon, bool hybridOnlineBatch);
    void exportState(json::Value *jsonDoc) const;
    void importState(const json::Value &jsonDoc);
protected:
    void _updateWeights();
    void _armUpdate();
    // the family's two calls (LambOptimizer names its own) and its name in the messages about autosave files
    virtual int _armCall(real_t lr);
    virtual int _layerCall(cn_layer *layer, real_t lr);
    virtual const char *_name() const { return "adam"; }
    real_t m_learningRate, m_beta1, m_beta2, m_epsilon;
    int64_t m_step;                 // updates applied so far
private:
    bool m_armed;                   // _armUpdate() has counted and armed the update _updateWeights() is about to complete
};

// LAMB (include/currennt_hip.h, section LAMB): Adam's state, options, seams and autosave members, the cn_lamb_* calls in place of
// the cn_adam_* ones, and the trust bounds, which travel with the autosave beside the member "lamb_optimizer": true.
class LambOptimizer : public AdamOptimizer {
public:
    LambOptimizer(NeuralNetwork &neuralNetwork, data_sets::DataSet &trainingSet, data_sets::DataSet &validationSet,
                  data_sets::DataSet &testSet, int maxEpochs, int maxEpochsNoBest, int validateEvery, int testEvery,
                  real_t learningRate, real_t beta1, real_t beta2, real_t epsilon, real_t minTrust, real_t maxTrust, bool hybridOnlineBatch);
    void exportState(json::Value *jsonDoc) const;
    void importState(const json::Value &jsonDoc);
    real_t minTrust() const { return m_minTrust; }
    real_t maxTrust() const { return m_maxTrust; }
    // the smallest and the largest trust ratio of the last update, with the layers that had them (one synchronising read per layer)
    struct TrustRange { float min, max; std::string minLayer, maxLayer; };
    TrustRange trustRange();
protected:
    int _armCall(real_t lr);
    int _layerCall(cn_layer *layer, real_t lr);
    const char *_name() const { return "lamb"; }
private:
    real_t m_minTrust, m_maxTrust;
};

}  // namespace optimizers
}  // namespace currennt_hip
