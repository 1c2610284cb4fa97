#include "Configuration.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace currennt_hip {

namespace {

std::string trim(const std::string &s)
{
    size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? std::string() : s.substr(a, b - a + 1);
}
bool toBool(const std::string &key, const std::string &v)
{
    if (v == "true" || v == "1" || v == "on" || v == "yes") return true;
    if (v == "false" || v == "0" || v == "off" || v == "no") return false;
    throw std::runtime_error("Error while parsing the command line and/or options file: invalid value '" + v + "' for option '" + key + "'");
}
std::vector<std::string> splitList(const std::string &v)      // Configuration.cpp:219-226 (',' and ';' separated lists)
{
    std::vector<std::string> out;
    std::string cur;
    for (size_t i = 0; i <= v.size(); ++i) {
        if (i == v.size() || v[i] == ',' || v[i] == ';') { if (!trim(cur).empty()) out.push_back(trim(cur)); cur.clear(); }
        else cur += v[i];
    }
    return out;
}

}  // namespace

const char *Configuration::usage()
{
    return "Usage: currennt_hip [options] [options-file]\n"
           "  common:   --network F --parallel_sequences N --random_seed N --cuda B(ignored) --list_devices B\n"
           "            --precision f32|bf16|bf16x3 --device N\n"
           "            --deterministic B (gradient sums in a fixed order: bit-identical runs; default true for f32 / bf16x3)\n"
           "            --gpus N (training only: data-parallel over N GPUs of this node, devices --device .. --device+N-1;\n"
           "                      parallel_sequences is per GPU; gradients are summed with RCCL)\n"
           "  training: --train B --stochastic B (= --hybrid_online_batch) --shuffle_fractions B --shuffle_sequences B\n"
           "            --max_epochs N --max_epochs_no_best N --validate_every N --test_every N --learning_rate X\n"
           "            --optimizer steepest_descent|adam|lamb (adam, lamb: --learning_rate is the step size, --momentum is ignored)\n"
           "            --adam_beta1 X --adam_beta2 X --adam_epsilon X (defaults 0.9, 0.999, 1e-8; lamb uses them too)\n"
           "            --lamb_min_trust X --lamb_max_trust X (lamb: every layer's step is scaled by |w| / |u| of that layer, kept\n"
           "                      inside these bounds; --weight_decay enters lamb's direction u; defaults 0 and 0 = unbounded)\n"
           "            --max_grad_norm X (clip every update's gradient to this global L2 norm; a step with a non-finite gradient is\n"
           "                      skipped; default 0 = off)\n"
           "            --weight_decay X (decoupled weight decay, AdamW-style, for both optimizers: every input and recurrent weight\n"
           "                      shrinks by learning rate * X of itself per update; biases and peepholes do not; default 0 = off)\n"
           "            --learning_rate_warmup_updates N (update k <= N runs at k / N of the learning rate; default 0 = off)\n"
           "            --learning_rate_decay F --learning_rate_decay_patience E --learning_rate_min M (after E epochs in a row\n"
           "                      without a new lowest validation error -- training error without a validation set -- the rate is\n"
           "                      multiplied by F, not below M; 0 < F <= 1, default 1 = off; E >= 1, default 1; M >= 0, default 0)\n"
           "            --weight_average_decay D (keep an exponential moving average of the weights, one step behind every update;\n"
           "                      validation, early stopping, trained_network.jsn and .best.jsn use it; 0 < D < 1, default 0 = off)\n"
           "            --weight_average_warmup B (step k >= 2 averages with min(D, k / (k + 9)); default true)\n"
           "            --weight_noise_sigma X (Gaussian noise on the weights the backward pass reads; default 0 = off)\n"
           "            --weight_noise_on_device B (generate that noise on the device from --random_seed, the epoch and the fraction\n"
           "                      index: no host copies, the update stays overlapped, --continue resumes the same noise; default false)\n"
           "            --input_noise_sigma X (Gaussian noise on the input patterns of the training set and of --ff_input_file; default 0)\n"
           "            --input_noise_on_device B (generate that noise on the device from --random_seed, the epoch and the fraction\n"
           "                      index instead of on the loader thread; --continue resumes the same noise; default false)\n"
           "            --spec_augment_freq_masks N --spec_augment_freq_width F --spec_augment_time_masks N --spec_augment_time_width W\n"
           "            --spec_augment_time_ratio X (SpecAugment on the training fractions, on the device: N masks (0..8) of up to F\n"
           "                      features / W frames each set to 0; a time mask is at most X (0..1, default 1) of its sequence)\n"
           "            --input_frame_skip K (low-frame-rate input, every set and --ff_input_file: the network runs on every K-th frame,\n"
           "                      each with its --input_left_context / --input_right_context frames spliced around it; 1..16, default 1)\n"
           "            --input_splice_on_device B (upload the frames unspliced at source rate and splice / skip where a fraction is\n"
           "                      re-laid out on the device; contexts of at most 32 frames per side; default false.  With a skip above\n"
           "                      1, --input_noise_on_device and --spec_augment_* need it: they belong to the source frames)\n"
           "            --momentum X --save_network F --train_file F[,F] --val_file F --test_file F --truncate_seq N\n"
           "            --train_fraction X --val_fraction X --test_fraction X\n"
           "            --weights_dist uniform|normal --weights_uniform_min X --weights_uniform_max X\n"
           "            --weights_normal_sigma X --weights_normal_mean X\n"
           "            --ctc_train_label_errors B (ctc nets: the training column shows the label error rate of best-path decoding of\n"
           "                      the training pass's own posteriors, dropout and all, counted on the device; default false: '-')\n"
           "  forward:  --ff_input_file F --ff_output_file F --ff_output_format single_csv|csv|htk|ctc_labels\n"
           "                      (ctc_labels, ctc nets only: --ff_output_file is one text file with a line `<seqTag>;<l0> <l1> ...`\n"
           "                      per sequence, the best-path decoding; labels by name when the input file has a `labels` variable)\n"
           "            --ff_output_kind N --feature_period X --revert_std B\n";
}

void Configuration::apply(const std::string &key, const std::string &v)
{
    if (key != "continue" && v.find_first_of(";\"\\") == std::string::npos) m_serializedOptions += key + "=" + v + ";";
    if (key == "network") m_networkFile = v;
    else if (key == "cuda") (void)toBool(key, v);                       // accepted for compatibility; this build always runs on the MI355X
    else if (key == "list_devices") m_listDevices = toBool(key, v);
    else if (key == "parallel_sequences") m_parallelSequences = atoi(v.c_str());
    else if (key == "random_seed") m_randomSeed = (unsigned)strtoul(v.c_str(), 0, 10);
    else if (key == "ff_output_format") {
        if (v == "single_csv") m_feedForwardFormat = FORMAT_SINGLE_CSV;
        else if (v == "csv") m_feedForwardFormat = FORMAT_CSV;
        else if (v == "htk") m_feedForwardFormat = FORMAT_HTK;
        else if (v == "ctc_labels") m_feedForwardFormat = FORMAT_CTC_LABELS;
        else throw std::runtime_error("Error while parsing the command line and/or options file: unknown output format '" + v + "'");
    }
    else if (key == "ff_output_file") m_feedForwardOutputFile = v;
    else if (key == "ff_output_kind") m_outputFeatureKind = atoi(v.c_str());
    else if (key == "feature_period") m_featurePeriod = (real_t)atof(v.c_str());
    else if (key == "ff_input_file") m_feedForwardInputFiles = splitList(v);
    else if (key == "revert_std") m_revertStd = toBool(key, v);
    else if (key == "train") m_trainingMode = toBool(key, v);
    else if (key == "stochastic" || key == "hybrid_online_batch") m_hybridOnlineBatch = toBool(key, v);
    else if (key == "shuffle_fractions") m_shuffleFractions = toBool(key, v);
    else if (key == "shuffle_sequences") m_shuffleSequences = toBool(key, v);
    else if (key == "max_epochs") m_maxEpochs = atoi(v.c_str());
    else if (key == "max_epochs_no_best") m_maxEpochsNoBest = atoi(v.c_str());
    else if (key == "validate_every") m_validateEvery = atoi(v.c_str());
    else if (key == "test_every") m_testEvery = atoi(v.c_str());
    else if (key == "optimizer") { if (v == "adam" || v == "lamb" || v == "steepest_descent") m_optimizer = v; else throw std::runtime_error("Error while parsing the command line and/or options file: unknown optimizer '" + v + "' (steepest_descent, adam or lamb)"); }
    else if (key == "lamb_min_trust" || key == "lamb_max_trust") {
        real_t &bound = key == "lamb_min_trust" ? m_lambMinTrust : m_lambMaxTrust;
        bound = (real_t)atof(v.c_str());
        if (!(bound >= 0) || std::isinf(bound))
            throw std::runtime_error("Error while parsing the command line and/or options file: --" + key + " must be finite and >= 0 (0 = off)");
    }
    else if (key == "learning_rate") m_learningRate = (real_t)atof(v.c_str());
    else if (key == "momentum") m_momentum = (real_t)atof(v.c_str());
    else if (key == "adam_beta1") m_adamBeta1 = (real_t)atof(v.c_str());
    else if (key == "adam_beta2") m_adamBeta2 = (real_t)atof(v.c_str());
    else if (key == "adam_epsilon") m_adamEpsilon = (real_t)atof(v.c_str());
    else if (key == "max_grad_norm") {
        m_maxGradNorm = (real_t)atof(v.c_str());
        if (!(m_maxGradNorm >= 0) || std::isinf(m_maxGradNorm))
            throw std::runtime_error("Error while parsing the command line and/or options file: --max_grad_norm must be finite and >= 0 (0 = off)");
    }
    else if (key == "weight_decay") {
        m_weightDecay = (real_t)atof(v.c_str());
        if (!(m_weightDecay >= 0) || std::isinf(m_weightDecay))
            throw std::runtime_error("Error while parsing the command line and/or options file: --weight_decay must be finite and >= 0 (0 = off)");
    }
    else if (key == "learning_rate_warmup_updates") {
        m_lrWarmupUpdates = atoll(v.c_str());
        if (m_lrWarmupUpdates < 0) throw std::runtime_error("Error while parsing the command line and/or options file: --learning_rate_warmup_updates must be >= 0");
    }
    else if (key == "learning_rate_decay") {
        m_lrDecay = atof(v.c_str());
        if (!(m_lrDecay > 0 && m_lrDecay <= 1))
            throw std::runtime_error("Error while parsing the command line and/or options file: --learning_rate_decay must be in (0, 1] (1 = off)");
    }
    else if (key == "learning_rate_decay_patience") {
        m_lrDecayPatience = atoi(v.c_str());
        if (m_lrDecayPatience < 1) throw std::runtime_error("Error while parsing the command line and/or options file: --learning_rate_decay_patience must be >= 1");
    }
    else if (key == "learning_rate_min") {
        m_lrMin = atof(v.c_str());
        if (!(m_lrMin >= 0) || std::isinf(m_lrMin))
            throw std::runtime_error("Error while parsing the command line and/or options file: --learning_rate_min must be finite and >= 0");
    }
    else if (key == "weight_average_decay") {
        m_weightAverageDecay = (real_t)atof(v.c_str());
        if (!(m_weightAverageDecay >= 0 && m_weightAverageDecay < 1))
            throw std::runtime_error("Error while parsing the command line and/or options file: --weight_average_decay must be in [0, 1) (0 = off)");
    }
    else if (key == "weight_average_warmup") m_weightAverageWarmup = toBool(key, v);
    else if (key == "save_network") m_trainedNetwork = v;
    else if (key == "train_file") m_trainingFiles = splitList(v);
    else if (key == "val_file") m_validationFiles = splitList(v);
    else if (key == "test_file") m_testFiles = splitList(v);
    else if (key == "train_fraction") m_trainingFraction = (real_t)atof(v.c_str());
    else if (key == "val_fraction") m_validationFraction = (real_t)atof(v.c_str());
    else if (key == "test_fraction") m_testFraction = (real_t)atof(v.c_str());
    else if (key == "truncate_seq") m_truncSeqLength = atoi(v.c_str());
    else if (key == "weights_dist") {
        if (v == "uniform") m_weightsNormal = false; else if (v == "normal") m_weightsNormal = true;
        else throw std::runtime_error("Error while parsing the command line and/or options file: unknown weights distribution '" + v + "'");
    }
    else if (key == "weights_uniform_min") m_weightsUniformMin = (real_t)atof(v.c_str());
    else if (key == "weights_uniform_max") m_weightsUniformMax = (real_t)atof(v.c_str());
    else if (key == "weights_normal_sigma") m_weightsNormalSigma = (real_t)atof(v.c_str());
    else if (key == "weights_normal_mean") m_weightsNormalMean = (real_t)atof(v.c_str());
    else if (key == "precision") {
        if (v == "f32" || v == "fp32") m_precision = CN_PREC_F32; else if (v == "bf16") m_precision = CN_PREC_BF16;
        else if (v == "bf16x3") m_precision = CN_PREC_BF16X3;
        else throw std::runtime_error("Error while parsing the command line and/or options file: unknown precision '" + v + "'");
    }
    else if (key == "deterministic") m_deterministic = toBool(key, v) ? 1 : 0;
    else if (key == "device") m_device = atoi(v.c_str());
    else if (key == "gpus") { m_gpus = atoi(v.c_str()); if (m_gpus < 1) throw std::runtime_error("Error while parsing the command line and/or options file: --gpus must be >= 1"); }
    else if (key == "dp_rank") m_dpRank = atoi(v.c_str());
    else if (key == "dp_world") m_dpWorld = atoi(v.c_str());
    else if (key == "dump_fractions") m_dumpFractions = toBool(key, v);
    else if (key == "dump_labels") m_dumpLabels = toBool(key, v);
    else if (key == "ctc_train_label_errors") m_ctcTrainLabelErrors = toBool(key, v);
    else if (key == "dump_epochs") m_dumpEpochs = std::max(1, atoi(v.c_str()));
    else if (key == "input_noise_sigma") m_inputNoiseSigma = (real_t)atof(v.c_str());
    else if (key == "weight_noise_sigma") m_weightNoiseSigma = (real_t)atof(v.c_str());
    else if (key == "weight_noise_on_device") m_weightNoiseOnDevice = toBool(key, v);
    else if (key == "input_noise_on_device") m_inputNoiseOnDevice = toBool(key, v);
    else if (key == "spec_augment_freq_masks" || key == "spec_augment_time_masks") {
        const int n = atoi(v.c_str());
        if (n < 0 || n > 8) throw std::runtime_error("Error while parsing the command line and/or options file: --" + key + " must be in 0..8");
        (key == "spec_augment_freq_masks" ? m_specFreqMasks : m_specTimeMasks) = n;
    }
    else if (key == "spec_augment_freq_width" || key == "spec_augment_time_width") {
        const int w = atoi(v.c_str());
        if (w < 0) throw std::runtime_error("Error while parsing the command line and/or options file: --" + key + " must be >= 0");
        (key == "spec_augment_freq_width" ? m_specFreqWidth : m_specTimeWidth) = w;
    }
    else if (key == "spec_augment_time_ratio") {
        m_specTimeRatio = (real_t)atof(v.c_str());
        if (!(m_specTimeRatio >= 0 && m_specTimeRatio <= 1))
            throw std::runtime_error("Error while parsing the command line and/or options file: --spec_augment_time_ratio must be in 0..1");
    }
    else if (key == "input_left_context") m_inputLeftContext = atoi(v.c_str());
    else if (key == "input_right_context") m_inputRightContext = atoi(v.c_str());
    else if (key == "output_time_lag") m_outputTimeLag = atoi(v.c_str());
    else if (key == "input_frame_skip") {
        m_inputFrameSkip = atoi(v.c_str());
        if (m_inputFrameSkip < 1 || m_inputFrameSkip > 16)
            throw std::runtime_error("Error while parsing the command line and/or options file: --input_frame_skip must be in 1..16");
    }
    else if (key == "input_splice_on_device") m_inputSpliceOnDevice = toBool(key, v);
    else if (key == "autosave") m_autosave = toBool(key, v);
    else if (key == "autosave_best") m_autosaveBest = toBool(key, v);
    else if (key == "autosave_prefix") m_autosavePrefix = v;
    else if (key == "continue") m_continueFile = v;
    else if (key == "cache_path") { /* accepted, unused: sequences are kept in RAM instead of a cache file */ }
    else throw std::runtime_error("Error while parsing the command line and/or options file: unknown option '" + key + "'");
}

Configuration::Configuration(int argc, const char *argv[])
{
    std::vector<std::pair<std::string, std::string> > cli;
    std::string optionsFile;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--help" || a == "-h") { m_help = true; continue; }
        if (a.compare(0, 2, "--") == 0) {
            std::string key = a.substr(2), val;
            size_t eq = key.find('=');
            if (eq != std::string::npos) { val = key.substr(eq + 1); key = key.substr(0, eq); }
            else if (i + 1 < argc) val = argv[++i];
            else throw std::runtime_error("Error while parsing the command line and/or options file: missing value for '" + key + "'");
            if (key == "options_file") optionsFile = val; else cli.push_back(std::make_pair(key, val));
        } else optionsFile = a;                                                  // positional options file, Configuration.cpp:192-194
    }
    if (!optionsFile.empty()) {
        std::ifstream f(optionsFile.c_str());
        if (!f.good()) throw std::runtime_error("Error while parsing the command line and/or options file: cannot open '" + optionsFile + "'");
        std::string line;
        while (std::getline(f, line)) {
            size_t hash = line.find('#');
            if (hash != std::string::npos) line = line.substr(0, hash);
            size_t eq = line.find('=');
            if (eq == std::string::npos) continue;
            apply(trim(line.substr(0, eq)), trim(line.substr(eq + 1)));
        }
    }
    // --continue: the options stored in the autosave file come first (Configuration.cpp:236-248)
    for (size_t i = 0; i < cli.size(); ++i)
        if (cli[i].first == "continue") {
            std::ifstream f(cli[i].second.c_str());
            if (!f.good()) throw std::runtime_error("Error while restoring configuration from autosave file: cannot open '" + cli[i].second + "'");
            std::stringstream ss; ss << f.rdbuf();
            const std::string text = ss.str(), tag = "\"configuration\"";
            size_t p = text.find(tag);
            if (p != std::string::npos && (p = text.find('"', text.find(':', p + tag.size()))) != std::string::npos) {
                size_t e = text.find('"', p + 1);
                std::vector<std::string> kv;
                std::string cur;
                for (size_t k = p + 1; k <= e && e != std::string::npos; ++k) {
                    if (k == e || text[k] == ';') { if (!cur.empty()) kv.push_back(cur); cur.clear(); } else cur += text[k];
                }
                for (size_t k = 0; k < kv.size(); ++k) {
                    size_t eq = kv[k].find('=');
                    if (eq != std::string::npos && kv[k].substr(0, eq) != "continue") apply(kv[k].substr(0, eq), kv[k].substr(eq + 1));
                }
            }
        }
    if (const char *dev = getenv("CURRENNT_CUDA_DEVICE")) m_device = atoi(dev);       // main.cpp:527-531 (kept under its old name)
    for (size_t i = 0; i < cli.size(); ++i) apply(cli[i].first, cli[i].second);   // command line wins
    if (m_parallelSequences < 1) throw std::runtime_error("Error while parsing the command line and/or options file: parallel_sequences must be >= 1");
    // The device's augmentation belongs to the SOURCE frames (include/currennt_hip.h, section Input augmentation).  Fractions the
    // host has already skipped frames of carry network-rate rows, where that rule cannot be applied: it takes the device's splice.
    if (m_inputFrameSkip > 1 && !m_inputSpliceOnDevice && ((m_inputNoiseOnDevice && m_inputNoiseSigma > 0) || specAugment()))
        throw std::runtime_error("Error while parsing the command line and/or options file: --input_noise_on_device and --spec_augment_* "
                                 "with --input_frame_skip above 1 need --input_splice_on_device true");
    if (m_inputSpliceOnDevice && (m_inputLeftContext < 0 || m_inputLeftContext > 32 || m_inputRightContext < 0 || m_inputRightContext > 32))
        throw std::runtime_error("Error while parsing the command line and/or options file: --input_splice_on_device true needs "
                                 "--input_left_context and --input_right_context in 0..32");
}

}  // namespace currennt_hip
