// In-memory data set and fraction packer: the host objects of currennt_lib/src/data_sets/
// {DataSet,DataSetFraction}.{hpp,cpp} for NetCDF-3 classic files (the reference goes through
// libnetcdf and a /tmp cache file; sequences here are kept in RAM).
#pragma once

#include <future>
#include <random>
#include <string>
#include <vector>

#include "../Types.hpp"

namespace currennt_hip {
namespace data_sets {

// one mini batch of parallel sequences (DataSetFraction.hpp:40-66)
class DataSetFraction {
public:
    struct seq_info_t { int originalSeqIdx; int length; std::string seqTag; };

    int inputPatternSize() const { return m_inputPatternSize; }
    int outputPatternSize() const { return m_outputPatternSize; }
    int maxSeqLength() const { return m_maxSeqLength; }
    int minSeqLength() const { return m_minSeqLength; }
    // The lengths and pattern types every layer behind the input re-layout sees.  They are the fraction's own unless it is a
    // source-rate fraction for the device to splice and skip (Augment::spliceOnDevice): then maxSeqLength() / minSeqLength() /
    // patTypes() / inputs() are what is uploaded and these are what include/currennt_hip.h, section Input splicing and frame
    // skipping, derives from them.  seqInfo(i).length is always the network-rate length.
    bool sourceRate() const { return !m_netPatTypes.empty(); }
    int networkMaxSeqLength() const { return m_netPatTypes.empty() ? m_maxSeqLength : m_netMaxSeqLength; }
    int networkMinSeqLength() const { return m_netPatTypes.empty() ? m_minSeqLength : m_netMinSeqLength; }
    const Hip::pattype_vector &networkPatTypes() const { return m_netPatTypes.empty() ? m_patTypes : m_netPatTypes; }
    int numSequences() const { return (int)m_seqInfo.size(); }
    const seq_info_t &seqInfo(int seqIdx) const { return m_seqInfo.at(seqIdx); }
    const Hip::pattype_vector &patTypes() const { return m_patTypes; }
    const Hip::real_vector &inputs() const { return m_inputs; }
    const Hip::real_vector &outputs() const { return m_outputs; }
    const Hip::int_vector &targetClasses() const { return m_targetClasses; }
    // classification data: the label sequence of each sequence of the fraction, slot by slot; what a ctc post output layer trains
    // against (no counterpart in the reference).  Transcription data (DataSet::hasTranscripts): the sequence's transcript from
    // `targetStrings`, repeats and the empty sequence included.  Otherwise its per-frame target classes with every run collapsed
    // (a a a b b a -> a b a), where a label that repeats without another one in between cannot be expressed.
    const std::vector<std::vector<int> > &labelSeqs() const { return m_labelSeqs; }

private:
    friend class DataSet;
    int m_inputPatternSize = 0, m_outputPatternSize = 0, m_maxSeqLength = 0, m_minSeqLength = 0, m_netMaxSeqLength = 0, m_netMinSeqLength = 0;
    Hip::pattype_vector m_netPatTypes;
    std::vector<seq_info_t> m_seqInfo;
    Hip::real_vector m_inputs, m_outputs;
    Hip::pattype_vector m_patTypes;
    Hip::int_vector m_targetClasses;
    std::vector<std::vector<int> > m_labelSeqs;
};

// what the reference pulls from Configuration::instance() inside _makeFractionTask / _addNoise
// (DataSet.cpp:252-265,302-305): Gaussian input noise, context splicing, output time lag
// frameSkip K (--input_frame_skip): the fractions keep frames K * j of every sequence, each with its context spliced around it and
// the targets of frame K * j (the lag applies at source rate), as sequences of ceil(length / K) frames.  spliceOnDevice
// (--input_splice_on_device): the fractions are emitted unspliced at source rate instead, for cn_ctx_set_input_splice
struct Augment { real_t noiseDeviation = 0; int contextLeft = 0, contextRight = 0, outputLag = 0, frameSkip = 1; bool spliceOnDevice = false; };

class DataSet {
public:
    typedef data_sets::Augment Augment;
    // labelsBegin / labelCount: the sequence's transcript in m_transcriptData (transcription data only)
    struct sequence_t { int originalSeqIdx; int length; std::string seqTag; size_t inputsBegin; size_t targetsBegin; size_t labelsBegin; int labelCount; };

    DataSet();                                              // empty set (DataSet.cpp:429-442)
    // DataSet.cpp:443-606; `sortByLength` = Configuration::trainingMode() there (:603-605)
    DataSet(const std::vector<std::string> &ncfiles, int parSeq, real_t fraction, int truncSeqLength,
            bool fracShuf, bool seqShuf, bool sortByLength, unsigned randomSeed, const Augment &augment = Augment());
    ~DataSet();
    DataSet(const DataSet &) = delete;
    DataSet &operator=(const DataSet &) = delete;

    // Data-parallel training: a GLOBAL fraction is world * parallelSequences consecutive sequences of the
    // (sorted / shuffled) list and rank r packs sequences r, r + world, r + 2 world, ... of it -- round-robin over the
    // length-sorted list keeps the ranks' T nearly equal.  Every rank sees the same number of fractions per epoch; a rank
    // whose share of the last global fraction is empty gets an all-dummy fraction (one time step of PATTYPE_NONE), which
    // contributes zero error and zero gradients but keeps the collectives matched.  Shuffles use the same seed on every
    // rank, so all ranks permute alike.
    void setShard(int rank, int world);
    bool isClassificationData() const { return m_isClassificationData; }
    bool empty() const { return m_totalTimesteps == 0; }
    // next fraction, or false once per epoch after the last one (DataSet.cpp:632-668)
    bool getNextFraction(DataSetFraction *frac);
    int totalSequences() const { return m_totalSequences; }
    int totalTimesteps() const { return m_totalTimesteps; }
    // the frames the network sees: the sum of ceil(length / frameSkip) over the sequences, the pieces of --truncate_seq each on
    // its own (= totalTimesteps() at a skip of 1).  What a per-frame error rate is taken over.
    int totalNetworkTimesteps() const { return m_totalNetworkTimesteps; }
    // ... behind context layers whose strides multiply to `stride`: the sum of ceil(ceil(length / frameSkip) / stride)
    int totalNetworkTimesteps(int stride) const;
    int minSeqLength() const { return m_minSeqLength; }
    int maxSeqLength() const { return m_maxSeqLength; }
    int inputPatternSize() const { return m_inputPatternSize; }                        // per frame, before context splicing
    int fractionInputPatternSize() const { return m_inputPatternSize * (m_augment.contextLeft + m_augment.contextRight + 1); }
    int outputPatternSize() const { return m_outputPatternSize; }
    int numLabels() const { return m_numLabels; }                                     // classification data: the numLabels dimension
    // Transcription data (the layout of RNNLIB's CTC corpora): the files have `targetStrings(numSeqs, maxTargStringLength)`, one
    // string of label names per sequence, and the alphabet `labels(numLabels, maxLabelLength)`; the label sequences of the fractions
    // are the transcripts.  Such files need no `targetClasses`: hasTargetClasses() says whether they have them (the fractions'
    // targetClasses are all -1 when not, and only a ctc post output layer can train on the set).
    bool hasTranscripts() const { return m_hasTranscripts; }
    bool hasTargetClasses() const { return m_hasTargetClasses; }
    // --truncate_seq cut the sequences of a set with transcripts into pieces: labelSeqs() of its fractions mean nothing (every piece
    // carries the whole transcript), so the driver refuses a ctc net and --dump_labels on it
    bool transcriptsCut() const { return m_transcriptsCut; }
    // the `labels` variable of the first file, row k the name of label k; empty when the file has none
    const std::vector<std::string> &labelNames() const { return m_labelNames; }
    const Hip::real_vector &outputMeans() const { return m_outputMeans; }
    const Hip::real_vector &outputStdevs() const { return m_outputStdevs; }
    // what the loader thread has spent packing fractions so far (noise and splicing included) and how many it packed: read
    // between epochs by the driver's CN_LOADER_TIME hook (tools/augment_cost.py)
    double loaderSeconds() const { return m_loaderSeconds; }
    long loaderFractions() const { return m_loaderFractions; }

private:
    double m_loaderSeconds = 0;
    long m_loaderFractions = 0;
    bool m_fractionShuffling = false, m_sequenceShuffling = false, m_isClassificationData = false, m_hasTranscripts = false, m_hasTargetClasses = false, m_transcriptsCut = false;
    std::vector<std::string> m_labelNames;
    Hip::int_vector m_transcriptData;
    int m_parallelSequences = 0, m_totalSequences = 0, m_totalTimesteps = 0, m_totalNetworkTimesteps = 0, m_minSeqLength = 0, m_maxSeqLength = 0,
        m_inputPatternSize = 0, m_outputPatternSize = 0, m_numLabels = 0, m_curFirstSeqIdx = -1, m_rank = 0, m_world = 1;
    unsigned m_rngState = 0;
    Hip::real_vector m_outputMeans, m_outputStdevs, m_inputData, m_targetData;
    Hip::int_vector m_classData;
    std::vector<sequence_t> m_sequences;

    Augment m_augment;
    std::mt19937 m_noiseGen;
    // one fraction is packed ahead on a worker thread while the GPU runs the current one
    // (the reference's boost::thread hand-over, DataSet.cpp:589,632-668)
    std::future<bool> m_prefetch;
    DataSetFraction m_next;
    bool produceNext(DataSetFraction *frac);

    static std::vector<int> truncatedPieces(int length, int trunc);   // --truncate_seq, DataSet.cpp:527-542
    void makeFraction(int firstSeqIdx, DataSetFraction *frac);        // _makeFractionTask, DataSet.cpp:300-414
    void shuffleSequences();                                          // :226-230
    void shuffleFractions();                                          // :232-250
    unsigned nextRandom(unsigned n);
};

}  // namespace data_sets
}  // namespace currennt_hip
