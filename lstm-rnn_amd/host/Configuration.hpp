// The handful of program options the hot path and its driver need (subset of
// currennt_lib/src/Configuration.cpp:120-190; same names, same defaults).  Options come from a
// `key = value` options file (positional argument or --options_file) and from `--key value` /
// `--key=value` on the command line; the command line wins (Configuration.cpp:192-217).
#pragma once

#include <map>
#include <string>
#include <vector>

#include "Types.hpp"

namespace currennt_hip {

class Configuration {
public:
    enum feedforwardformat_type_t { FORMAT_SINGLE_CSV, FORMAT_CSV, FORMAT_HTK, FORMAT_CTC_LABELS };

    Configuration(int argc, const char *argv[]);

    bool trainingMode() const { return m_trainingMode; }
    bool hybridOnlineBatch() const { return m_hybridOnlineBatch; }
    bool shuffleFractions() const { return m_shuffleFractions; }
    bool shuffleSequences() const { return m_shuffleSequences; }
    bool listDevices() const { return m_listDevices; }
    bool revertStd() const { return m_revertStd; }
    int parallelSequences() const { return m_parallelSequences; }
    int maxEpochs() const { return m_maxEpochs; }
    int maxEpochsNoBest() const { return m_maxEpochsNoBest; }
    int validateEvery() const { return m_validateEvery; }
    int testEvery() const { return m_testEvery; }
    int truncateSeqLength() const { return m_truncSeqLength; }
    int outputFeatureKind() const { return m_outputFeatureKind; }
    unsigned randomSeed() const { return m_randomSeed; }
    real_t learningRate() const { return m_learningRate; }
    real_t momentum() const { return m_momentum; }
    // --optimizer: "steepest_descent" (the reference's default, Configuration.cpp:152), "adam" or "lamb" (no counterpart there)
    const std::string &optimizer() const { return m_optimizer; }
    real_t adamBeta1() const { return m_adamBeta1; }
    real_t adamBeta2() const { return m_adamBeta2; }
    real_t adamEpsilon() const { return m_adamEpsilon; }
    // --lamb_min_trust / --lamb_max_trust: the bounds of lamb's per-layer trust ratio (include/currennt_hip.h, section LAMB); 0 = none
    real_t lambMinTrust() const { return m_lambMinTrust; }
    real_t lambMaxTrust() const { return m_lambMaxTrust; }
    // --max_grad_norm: bound on the global L2 norm of an update's gradient (include/currennt_hip.h, section Gradient clipping;
    // no counterpart in the reference); 0 = off
    real_t maxGradNorm() const { return m_maxGradNorm; }
    real_t weightDecay() const { return m_weightDecay; }
    long long learningRateWarmupUpdates() const { return m_lrWarmupUpdates; }
    double learningRateDecay() const { return m_lrDecay; }
    int learningRateDecayPatience() const { return m_lrDecayPatience; }
    double learningRateMin() const { return m_lrMin; }
    bool learningRateSchedule() const { return m_lrWarmupUpdates > 0 || m_lrDecay < 1.0; }
    // --weight_average_decay: decay of the exponential moving average of the weights that validation, early stopping and the saved
    // networks use (include/currennt_hip.h, section Weight averaging; no counterpart in the reference); 0 = off.
    // --weight_average_warmup: step k >= 2 uses min(decay, k / (k + 9))
    real_t weightAverageDecay() const { return m_weightAverageDecay; }
    bool weightAverageWarmup() const { return m_weightAverageWarmup; }
    real_t featurePeriod() const { return m_featurePeriod; }
    real_t trainingFraction() const { return m_trainingFraction; }
    real_t validationFraction() const { return m_validationFraction; }
    real_t testFraction() const { return m_testFraction; }
    real_t weightsDistributionUniformMin() const { return m_weightsUniformMin; }
    real_t weightsDistributionUniformMax() const { return m_weightsUniformMax; }
    real_t weightsDistributionNormalSigma() const { return m_weightsNormalSigma; }
    real_t weightsDistributionNormalMean() const { return m_weightsNormalMean; }
    bool weightsDistributionIsNormal() const { return m_weightsNormal; }
    feedforwardformat_type_t feedForwardFormat() const { return m_feedForwardFormat; }
    const std::string &networkFile() const { return m_networkFile; }
    const std::string &trainedNetworkFile() const { return m_trainedNetwork; }
    const std::string &feedForwardOutputFile() const { return m_feedForwardOutputFile; }
    const std::vector<std::string> &trainingFiles() const { return m_trainingFiles; }
    const std::vector<std::string> &validationFiles() const { return m_validationFiles; }
    const std::vector<std::string> &testFiles() const { return m_testFiles; }
    const std::vector<std::string> &feedForwardInputFiles() const { return m_feedForwardInputFiles; }
    cn_precision precision() const { return m_precision; }
    int device() const { return m_device; }
    // -1: the library's default (on for f32 / bf16x3, off for bf16); the library's "deterministic" option (cn_ctx_set_option)
    int deterministic() const { return m_deterministic; }
    // data-parallel training over `gpus` devices of this node, one process per GPU (no counterpart in the reference,
    // which drives one device: main.cpp:526-541); dpRank/dpWorld: shard of a host-only --dump_fractions run
    int gpus() const { return m_gpus; }
    int dpRank() const { return m_dpRank; }
    int dpWorld() const { return m_dpWorld; }
    bool help() const { return m_help; }
    bool dumpFractions() const { return m_dumpFractions; }
    bool dumpLabels() const { return m_dumpLabels; }          // --dump_fractions rows also print the label sequences' counts
    bool ctcTrainLabelErrors() const { return m_ctcTrainLabelErrors; }   // ctc: the training column shows the training pass's label error rate
    int dumpEpochs() const { return m_dumpEpochs; }
    // data/noise options of Configuration.cpp:139-146,171-176
    real_t inputNoiseSigma() const { return m_inputNoiseSigma; }
    real_t weightNoiseSigma() const { return m_weightNoiseSigma; }
    // --weight_noise_on_device: the noise of --weight_noise_sigma is generated on the device (include/currennt_hip.h, section
    // Weight noise) instead of drawn on the host and uploaded; default false
    bool weightNoiseOnDevice() const { return m_weightNoiseOnDevice; }
    // --input_noise_on_device: the noise of --input_noise_sigma is generated on the device where a fraction is re-laid out
    // (include/currennt_hip.h, section Input augmentation) instead of drawn by the data set's loader thread; default false
    bool inputNoiseOnDevice() const { return m_inputNoiseOnDevice; }
    // --spec_augment_*: SpecAugment's masks on the training fractions (same section); the ratio is handed over in permille
    int specAugmentFreqMasks() const { return m_specFreqMasks; }
    int specAugmentFreqWidth() const { return m_specFreqWidth; }
    int specAugmentTimeMasks() const { return m_specTimeMasks; }
    int specAugmentTimeWidth() const { return m_specTimeWidth; }
    real_t specAugmentTimeRatio() const { return m_specTimeRatio; }
    bool specAugment() const { return m_specFreqMasks > 0 || m_specTimeMasks > 0; }
    int inputLeftContext() const { return m_inputLeftContext; }
    int inputRightContext() const { return m_inputRightContext; }
    // --input_frame_skip K: the network runs on every K-th frame; --input_splice_on_device: the fractions go up unspliced at source
    // rate and the device splices and skips (include/currennt_hip.h, section Input splicing and frame skipping)
    int inputFrameSkip() const { return m_inputFrameSkip; }
    bool inputSpliceOnDevice() const { return m_inputSpliceOnDevice; }
    int outputTimeLag() const { return m_outputTimeLag; }
    // autosave options of Configuration.cpp:159-164
    bool autosave() const { return m_autosave; }
    bool autosaveBest() const { return m_autosaveBest; }
    const std::string &autosavePrefix() const { return m_autosavePrefix; }
    const std::string &continueFile() const { return m_continueFile; }
    // "key=value;..." of every option given (the reference serialises its boost variables map, Configuration.cpp:44-67)
    const std::string &serializedOptions() const { return m_serializedOptions; }
    static const char *usage();

private:
    int m_dumpEpochs = 1;
    bool m_dumpFractions = false, m_dumpLabels = false, m_ctcTrainLabelErrors = false, m_autosave = false, m_autosaveBest = false;
    real_t m_inputNoiseSigma = 0, m_weightNoiseSigma = 0;
    bool m_weightNoiseOnDevice = false, m_inputNoiseOnDevice = false;
    int m_specFreqMasks = 0, m_specFreqWidth = 0, m_specTimeMasks = 0, m_specTimeWidth = 0;
    real_t m_specTimeRatio = 1;
    int m_inputLeftContext = 0, m_inputRightContext = 0, m_outputTimeLag = 0, m_inputFrameSkip = 1;
    bool m_inputSpliceOnDevice = false;
    std::string m_autosavePrefix, m_continueFile, m_serializedOptions;
    bool m_help = false, m_trainingMode = false, m_hybridOnlineBatch = false, m_shuffleFractions = false,
         m_shuffleSequences = false, m_listDevices = false, m_revertStd = true, m_weightsNormal = false;
    int m_parallelSequences = 1, m_maxEpochs = -1, m_maxEpochsNoBest = 20, m_validateEvery = 1, m_testEvery = 1,
        m_truncSeqLength = 0, m_outputFeatureKind = 9, m_device = 0, m_gpus = 1, m_dpRank = 0, m_dpWorld = 1;
    unsigned m_randomSeed = 0;
    real_t m_learningRate = 1e-5f, m_momentum = 0.9f, m_featurePeriod = 10, m_trainingFraction = 1, m_validationFraction = 1,
           m_testFraction = 1, m_weightsUniformMin = -0.1f, m_weightsUniformMax = 0.1f, m_weightsNormalSigma = 0.1f, m_weightsNormalMean = 0;
    real_t m_adamBeta1 = 0.9f, m_adamBeta2 = 0.999f, m_adamEpsilon = 1e-8f;
    real_t m_lambMinTrust = 0, m_lambMaxTrust = 0;
    real_t m_maxGradNorm = 0;
    real_t m_weightDecay = 0;
    long long m_lrWarmupUpdates = 0;
    double m_lrDecay = 1.0, m_lrMin = 0.0;
    int m_lrDecayPatience = 1;
    real_t m_weightAverageDecay = 0;
    bool m_weightAverageWarmup = true;
    std::string m_optimizer = "steepest_descent";
    feedforwardformat_type_t m_feedForwardFormat = FORMAT_SINGLE_CSV;
    std::string m_networkFile = "network.jsn", m_trainedNetwork = "trained_network.jsn", m_feedForwardOutputFile = "ff_output.csv";
    std::vector<std::string> m_trainingFiles, m_validationFiles, m_testFiles, m_feedForwardInputFiles;
    cn_precision m_precision = CN_PREC_F32;
    int m_deterministic = -1;

    void apply(const std::string &key, const std::string &value);
};

}  // namespace currennt_hip
