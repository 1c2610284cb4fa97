#include "DataSet.hpp"

#include <algorithm>
#include <chrono>
#include <limits>
#include <stdexcept>

#include "../NetCdf3.hpp"

namespace currennt_hip {
namespace data_sets {

DataSet::DataSet() {}

// --truncate_seq (DataSet.cpp:527-542): a sequence is cut into pieces of `trunc` steps for as long as MORE than 1.5 x trunc
// steps remain; what remains then (0.5 .. 1.5 x trunc steps) is the last piece.  trunc <= 0: one piece.
std::vector<int> DataSet::truncatedPieces(int length, int trunc)
{
    std::vector<int> pieces;
    if (trunc > 0)
        for (; length > 1.5 * trunc; length -= trunc) pieces.push_back(trunc);
    if (length > 0) pieces.push_back(length);
    return pieces;
}

int DataSet::totalNetworkTimesteps(int stride) const
{
    if (stride <= 1) return m_totalNetworkTimesteps;
    const int K = m_augment.frameSkip;
    long total = 0;
    for (size_t i = 0; i < m_sequences.size(); ++i) total += ((m_sequences[i].length + K - 1) / K + stride - 1) / stride;
    return (int)total;
}

DataSet::~DataSet()
{
    if (m_prefetch.valid()) m_prefetch.wait();
}

DataSet::DataSet(const std::vector<std::string> &ncfiles, int parSeq, real_t fraction, int truncSeqLength,
                 bool fracShuf, bool seqShuf, bool sortByLength, unsigned randomSeed, const Augment &augment)
    : m_fractionShuffling(fracShuf), m_sequenceShuffling(seqShuf), m_parallelSequences(parSeq),
      m_minSeqLength(std::numeric_limits<int>::max()), m_maxSeqLength(std::numeric_limits<int>::min()),
      m_rngState(randomSeed ? randomSeed : 5489u), m_augment(augment), m_noiseGen(randomSeed)
{
    if (augment.contextLeft < 0 || augment.contextRight < 0 || augment.outputLag < 0)
        throw std::runtime_error("Negative input context / output time lag");
    if (augment.frameSkip < 1) throw std::runtime_error("Invalid input frame skip");
    if (fraction <= 0 || fraction > 1) throw std::runtime_error("Invalid fraction");        // DataSet.cpp:457-458
    bool firstFile = true;
    for (size_t fi = 0; fi < ncfiles.size(); ++fi) {
        NetCdf3File nc(ncfiles[fi]);
        const int maxSeqTagLength = nc.dimension("maxSeqTagLength");
        // transcription data: `targetStrings` beside the alphabet `labels`; `targetClasses` may be missing
        const bool transcripts = nc.hasVariable("targetStrings");
        if (transcripts && !(nc.hasDimension("numLabels") && nc.hasVariable("labels")))
            throw std::runtime_error("'" + ncfiles[fi] + "' has the variable 'targetStrings' but not the dimension 'numLabels' and the variable 'labels' its label names come from");
        if (firstFile) {                                                                       // :489-500
            m_isClassificationData = nc.hasDimension("numLabels");
            m_inputPatternSize = nc.dimension("inputPattSize");
            if (m_isClassificationData) { int numLabels = nc.dimension("numLabels"); m_numLabels = numLabels; m_outputPatternSize = (numLabels == 2 ? 1 : numLabels); }
            else m_outputPatternSize = nc.dimension("targetPattSize");
        } else {                                                                               // :502-515
            if (m_isClassificationData) {
                if (!nc.hasDimension("numLabels")) throw std::runtime_error("Cannot combine classification with regression NC");
                int numLabels = nc.dimension("numLabels");
                if (m_outputPatternSize != (numLabels == 2 ? 1 : numLabels)) throw std::runtime_error("Number of classes mismatch in NC files");
            } else if (m_outputPatternSize != nc.dimension("targetPattSize")) throw std::runtime_error("Number of targets mismatch in NC files");
            if (m_inputPatternSize != nc.dimension("inputPattSize")) throw std::runtime_error("Number of inputs mismatch in NC files");
        }
        if (firstFile) {
            m_hasTranscripts = transcripts;
            m_hasTargetClasses = nc.hasVariable("targetClasses");
        } else if (transcripts != m_hasTranscripts || (m_isClassificationData && nc.hasVariable("targetClasses") != m_hasTargetClasses))
            throw std::runtime_error("Cannot combine NC files with and without 'targetStrings' / 'targetClasses'");
        // --truncate_seq: a transcript cannot be cut with its frames.  Refused here when the transcripts are all the file has; a file
        // with targetClasses as well stays usable for every layer that reads those (transcriptsCut(): not for a ctc layer)
        if (transcripts && truncSeqLength > 0) {
            if (!nc.hasVariable("targetClasses"))
                throw std::runtime_error("--truncate_seq cannot be used with transcription data ('targetStrings' without 'targetClasses'): a transcript cannot be cut with its frames");
            m_transcriptsCut = true;
        }
        std::vector<std::string> names;
        if (nc.hasVariable("labels") && nc.hasDimension("numLabels") && (transcripts || nc.hasDimension("maxLabelLength"))) {
            const int maxLabelLength = nc.dimension("maxLabelLength");
            for (int k = 0; k < nc.dimension("numLabels"); ++k) {
                std::string name = nc.readString("labels", k, maxLabelLength);
                name.erase(name.find_last_not_of(" \t") + 1);                                   // (NUL- or space-padded)
                names.push_back(name);
            }
            if (firstFile) m_labelNames = names;
        }
        const int maxTargStringLength = transcripts ? nc.dimension("maxTargStringLength") : 0;
        int nSeq = nc.dimension("numSeqs");
        nSeq = std::max((int)((real_t)nSeq * fraction), 1);                                    // :518-520
        std::vector<int> lengths = nc.readInts("seqLengths", 0, nSeq);
        std::vector<sequence_t> sequences;
        for (int i = 0; i < nSeq; ++i) {
            m_totalTimesteps += lengths[i];
            std::string seqTag = nc.readString("seqTags", i, maxSeqTagLength);
            const std::vector<int> pieces = truncatedPieces(lengths[i], truncSeqLength);
            const size_t labelsBegin = m_transcriptData.size();
            if (transcripts) {                                                                  // label names separated by runs of blanks
                const std::string text = nc.readString("targetStrings", i, maxTargStringLength);
                for (size_t p = 0; p < text.size();) {
                    const size_t b = text.find_first_not_of(" \t\n", p);
                    if (b == std::string::npos) break;
                    const size_t e = std::min(text.find_first_of(" \t\n", b), text.size());
                    const std::string token = text.substr(b, e - b);
                    const size_t k = std::find(names.begin(), names.end(), token) - names.begin();
                    if (k == names.size())
                        throw std::runtime_error("Unknown label '" + token + "' in the target string of sequence '" + seqTag + "' ('" + ncfiles[fi] + "')");
                    m_transcriptData.push_back((int)k);
                    p = e;
                }
            }
            for (size_t k = 0; k < pieces.size(); ++k) {
                sequence_t seq;
                seq.originalSeqIdx = (int)k; seq.length = pieces[k]; seq.seqTag = seqTag;
                m_totalNetworkTimesteps += (pieces[k] + augment.frameSkip - 1) / augment.frameSkip;
                seq.inputsBegin = 0; seq.targetsBegin = 0;
                seq.labelsBegin = labelsBegin; seq.labelCount = (int)(m_transcriptData.size() - labelsBegin);
                sequences.push_back(seq);
            }
        }
        size_t frames = 0;
        for (size_t i = 0; i < sequences.size(); ++i) frames += sequences[i].length;
        // bulk read (the reference reads sequence by sequence into its cache file, :549-575)
        size_t inBase = m_inputData.size();
        { std::vector<float> x = nc.readFloats("inputs", 0, frames * m_inputPatternSize); m_inputData.insert(m_inputData.end(), x.begin(), x.end()); }
        size_t tgBase;
        if (m_isClassificationData) {
            tgBase = m_classData.size();
            if (m_hasTargetClasses) { std::vector<int> t = nc.readInts("targetClasses", 0, frames); m_classData.insert(m_classData.end(), t.begin(), t.end()); }
            else if (!transcripts) nc.readInts("targetClasses", 0, frames);                     // (says that the variable is missing, as ever)
        } else {
            tgBase = m_targetData.size();
            std::vector<float> t = nc.readFloats("targetPatterns", 0, frames * m_outputPatternSize); m_targetData.insert(m_targetData.end(), t.begin(), t.end());
        }
        size_t pos = 0;
        for (size_t i = 0; i < sequences.size(); ++i) {
            m_minSeqLength = std::min(m_minSeqLength, sequences[i].length);
            m_maxSeqLength = std::max(m_maxSeqLength, sequences[i].length);
            sequences[i].inputsBegin = inBase + pos * m_inputPatternSize;
            sequences[i].targetsBegin = tgBase + pos * (m_isClassificationData ? 1 : m_outputPatternSize);
            pos += sequences[i].length;
        }
        if (firstFile) {                                                                       // :577-588
            if (nc.hasVariable("outputMeans") && nc.hasVariable("outputStdevs")) {
                m_outputMeans = nc.readFloats("outputMeans", 0, m_outputPatternSize);
                m_outputStdevs = nc.readFloats("outputStdevs", 0, m_outputPatternSize);
            } else { m_outputMeans.assign(m_outputPatternSize, 0.0f); m_outputStdevs.assign(m_outputPatternSize, 1.0f); }
        }
        m_sequences.insert(m_sequences.end(), sequences.begin(), sequences.end());
        firstFile = false;
    }
    m_totalSequences = (int)m_sequences.size();
    if (sortByLength)                                                                          // :603-605 (std::sort, comp_seqs :164-167)
        std::sort(m_sequences.begin(), m_sequences.end(), [](const sequence_t &a, const sequence_t &b) { return a.length < b.length; });
}

void DataSet::setShard(int rank, int world)
{
    if (world < 1 || rank < 0 || rank >= world) throw std::runtime_error("Invalid data-parallel shard");
    if (m_prefetch.valid()) m_prefetch.wait();
    m_rank = rank; m_world = world;
}

unsigned DataSet::nextRandom(unsigned n)
{
    // The reference draws from boost::mt19937 (DataSet.cpp:169-181), which is not available here; a
    // xorshift generator seeded from --random_seed keeps shuffles reproducible per seed.
    m_rngState ^= m_rngState << 13; m_rngState ^= m_rngState >> 17; m_rngState ^= m_rngState << 5;
    return n ? m_rngState % n : 0;
}

void DataSet::shuffleSequences()
{
    for (size_t i = m_sequences.size(); i > 1; --i) std::swap(m_sequences[i - 1], m_sequences[nextRandom((unsigned)i)]);
}

void DataSet::shuffleFractions()
{
    std::vector<std::vector<sequence_t> > fractions;
    for (size_t i = 0; i < m_sequences.size(); ++i) {
        if (i % ((size_t)m_parallelSequences * m_world) == 0) fractions.resize(fractions.size() + 1);      // whole global fractions move
        fractions.back().push_back(m_sequences[i]);
    }
    for (size_t i = fractions.size(); i > 1; --i) std::swap(fractions[i - 1], fractions[nextRandom((unsigned)i)]);
    m_sequences.clear();
    for (size_t i = 0; i < fractions.size(); ++i) m_sequences.insert(m_sequences.end(), fractions[i].begin(), fractions[i].end());
}

void DataSet::makeFraction(int firstSeqIdx, DataSetFraction *frac)
{
    const int PS = m_parallelSequences;
    const int lag = m_augment.outputLag;                                                       // :302-305
    const int P = m_inputPatternSize;
    // --input_frame_skip: the fraction holds network frame j = source frame K * j of every sequence.  A source-rate fraction
    // (--input_splice_on_device) is packed with K = 1 and no context; the network-rate lengths and pattern types ride along.
    const bool source = m_augment.spliceOnDevice;
    const int skip = m_augment.frameSkip, K = source ? 1 : skip;
    const int ctxL = source ? 0 : m_augment.contextLeft, ctxR = source ? 0 : m_augment.contextRight, Pf = P * (ctxL + ctxR + 1);
    auto kept = [](int length, int k) { return (length + k - 1) / k; };
    *frac = DataSetFraction();
    frac->m_inputPatternSize = Pf;
    frac->m_outputPatternSize = m_outputPatternSize;
    frac->m_maxSeqLength = std::numeric_limits<int>::min();
    frac->m_minSeqLength = std::numeric_limits<int>::max();
    // this rank's sequences of the global fraction: firstSeqIdx + rank, + world, ... (world = 1: the reference's loop)
    auto globalIdx = [&](int i) { return firstSeqIdx + m_rank + i * m_world; };
    for (int i = 0; i < PS; ++i) {                                                             // :316-328
        const int seqIdx = globalIdx(i);
        if (seqIdx >= (int)m_sequences.size()) continue;
        frac->m_maxSeqLength = std::max(frac->m_maxSeqLength, kept(m_sequences[seqIdx].length, K));
        frac->m_minSeqLength = std::min(frac->m_minSeqLength, kept(m_sequences[seqIdx].length, K));
        DataSetFraction::seq_info_t si = { m_sequences[seqIdx].originalSeqIdx, kept(m_sequences[seqIdx].length, skip), m_sequences[seqIdx].seqTag };
        frac->m_seqInfo.push_back(si);
    }
    if (frac->m_seqInfo.empty()) { frac->m_maxSeqLength = 1; frac->m_minSeqLength = 0; }        // all-dummy fraction (setShard)
    const size_t slots = (size_t)frac->m_maxSeqLength * PS;
    if (source) {
        frac->m_netMaxSeqLength = kept(frac->m_maxSeqLength, skip); frac->m_netMinSeqLength = kept(frac->m_minSeqLength, skip);
        frac->m_netPatTypes.assign((size_t)frac->m_netMaxSeqLength * PS, (char)PATTYPE_NONE);
    }
    frac->m_inputs.assign(slots * Pf, 0.0f);                                                   // :330-336
    frac->m_patTypes.assign(slots, (char)PATTYPE_NONE);
    if (m_isClassificationData) frac->m_targetClasses.assign(slots, -1);
    else frac->m_outputs.assign(slots * m_outputPatternSize, 0.0f);
    std::vector<float> noisy;
    for (int i = 0; i < PS; ++i) {
        if (globalIdx(i) >= (int)m_sequences.size()) continue;
        const sequence_t &seq = m_sequences[globalIdx(i)];
        const float *src = m_inputData.data() + seq.inputsBegin;
        if (m_hasTranscripts)                                                                  // the label sequence: the transcript
            frac->m_labelSeqs.push_back(std::vector<int>(m_transcriptData.begin() + seq.labelsBegin, m_transcriptData.begin() + seq.labelsBegin + seq.labelCount));
        else if (m_isClassificationData) {                                                     // ... or the target classes, runs collapsed
            std::vector<int> labels;
            for (int t = 0; t < seq.length; ++t) {
                const int k = m_classData[seq.targetsBegin + t];
                if (labels.empty() || labels.back() != k) labels.push_back(k);
            }
            frac->m_labelSeqs.push_back(labels);
        }
        if (m_augment.noiseDeviation) {                                                        // _addNoise, :250-265
            // the reference draws from boost::mt19937 + boost::normal_distribution (absent here);
            // std::mt19937 seeded from --random_seed keeps runs reproducible per seed
            std::normal_distribution<real_t> dist((real_t)0, m_augment.noiseDeviation);
            noisy.assign(src, src + (size_t)seq.length * P);
            for (size_t k = 0; k < noisy.size(); ++k) noisy[k] += dist(m_noiseGen);
            src = noisy.data();
        }
        const int frames = kept(seq.length, K);
        for (int j = 0; j < frames; ++j) {
            const int t = K * j;
            const size_t slot = (size_t)j * PS + i;
            for (int off = -ctxL, k = 0; off <= ctxR; ++off, ++k) {                            // :346-366, edge frames are repeated
                const int ts = std::min(std::max(t + off, 0), seq.length - 1);
                std::copy(src + (size_t)ts * P, src + (size_t)(ts + 1) * P, frac->m_inputs.begin() + slot * Pf + (size_t)k * P);
            }
            if (m_isClassificationData) {                                                      // :372-380, class 0 before the lag
                if (m_hasTargetClasses) frac->m_targetClasses[slot] = t >= lag ? m_classData[seq.targetsBegin + (t - lag)] : 0;
            }                                                                                  // (transcripts alone: every class stays -1)
            else if (t >= lag)                                                                 // :383-397, 1.0 before the lag
                std::copy(m_targetData.begin() + seq.targetsBegin + (size_t)(t - lag) * m_outputPatternSize,
                          m_targetData.begin() + seq.targetsBegin + (size_t)(t - lag + 1) * m_outputPatternSize,
                          frac->m_outputs.begin() + slot * m_outputPatternSize);
            else std::fill_n(frac->m_outputs.begin() + slot * m_outputPatternSize, m_outputPatternSize, 1.0f);
            frac->m_patTypes[slot] = (char)(j == 0 ? PATTYPE_FIRST : (j == frames - 1 ? PATTYPE_LAST : PATTYPE_NORMAL));   // :400-407
        }
        if (source)
            for (int j = 0, n = kept(seq.length, skip); j < n; ++j)
                frac->m_netPatTypes[(size_t)j * PS + i] = (char)(j == 0 ? PATTYPE_FIRST : (j == n - 1 ? PATTYPE_LAST : PATTYPE_NORMAL));
    }
}

bool DataSet::produceNext(DataSetFraction *frac)
{
    if (m_curFirstSeqIdx == -1 || m_curFirstSeqIdx == 0) {       // start of an epoch: _makeFirstFractionTask, :416-427
        if (m_curFirstSeqIdx == -1) m_curFirstSeqIdx = 0;
        if (m_sequenceShuffling) shuffleSequences();
        if (m_fractionShuffling) shuffleFractions();
    }
    if (m_curFirstSeqIdx < (int)m_sequences.size()) {
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        makeFraction(m_curFirstSeqIdx, frac);
        m_loaderSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ++m_loaderFractions;
        m_curFirstSeqIdx += m_parallelSequences * m_world;
        return true;
    }
    m_curFirstSeqIdx = 0;                                        // :660-662
    return false;
}

bool DataSet::getNextFraction(DataSetFraction *frac)
{
    // :632-668: take the fraction the worker prepared and start the worker on the one after it.  After the
    // last fraction the worker's task only rewinds (returns false); the next epoch's shuffles run when that
    // epoch's first fraction is asked for, as in the reference.
    if (!m_prefetch.valid()) m_prefetch = std::async(std::launch::async, [this] { return produceNext(&m_next); });
    const bool ok = m_prefetch.get();
    if (ok) {
        std::swap(*frac, m_next);
        m_prefetch = std::async(std::launch::async, [this] { return produceNext(&m_next); });
    }
    return ok;
}

}  // namespace data_sets
}  // namespace currennt_hip
