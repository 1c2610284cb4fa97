// Learning-rate schedule of the optimizers: linear warm-up over the first updates, and a decay of the rate when the monitored
// error stalls (the "newbob" habit: halve it when validation stops improving).  Host arithmetic only -- the C ABI takes the rate
// per call -- and no dependency beyond the standard library, so that a stand-alone program can drive it
// (tests/schedule_main.cpp).  Cosine or cyclic schedules would go here.
//
// State: `updates` U, the update steps made (steps the clipping record skips still count: the library keeps no clock);
// `scale` s, starting at 1; `bad`, the epochs since the monitored error last improved; `lowest`, the lowest error seen.
// Update k = U + 1 runs at factor f = s * (N > 0 ? min(1, k / N) : 1), formed in double, and at rate (float)(rate * f).
// At the end of an epoch with a monitored error e:  e < lowest: lowest = e, bad = 0;  otherwise bad += 1 (an equal error is no
// improvement);  bad >= E:  s = max(s * F, M / learning_rate), bad = 0.
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>

namespace currennt_hip {
namespace optimizers {

class LearningRateSchedule {
public:
    struct State { int64_t updates; double scale; int bad; double lowest; };

    LearningRateSchedule() {}
    // warmupUpdates N >= 0 (0: none), decay 0 < F <= 1 (1: off), patience E >= 1, minRate M >= 0, learningRate: --learning_rate
    LearningRateSchedule(int64_t warmupUpdates, double decay, int patience, double minRate, double learningRate)
        : m_warmup(warmupUpdates), m_decay(decay), m_patience(patience), m_min(minRate), m_rate(learningRate) {}

    bool on() const { return m_warmup > 0 || m_decay < 1.0; }

    // the factor of update k = U + 1
    double factor() const
    {
        double f = m_state.scale;
        if (m_warmup > 0) f *= std::min(1.0, (double)(m_state.updates + 1) / (double)m_warmup);
        return f;
    }
    // `rate` (the global --learning_rate, or a layer's own) as the next update uses it
    float scaled(float rate) const { return (float)((double)rate * factor()); }
    float rate() const { return scaled((float)m_rate); }

    // one update step has been made
    void countUpdate() { ++m_state.updates; }

    // the end of an epoch that has a monitored error; returns whether the scale was lowered
    bool epochEnd(double error)
    {
        if (error < m_state.lowest) { m_state.lowest = error; m_state.bad = 0; return false; }
        if (++m_state.bad < m_patience) return false;
        m_state.bad = 0;
        const double before = m_state.scale;
        m_state.scale = std::max(m_state.scale * m_decay, m_rate > 0 ? m_min / m_rate : 0.0);
        return m_state.scale != before;
    }

    const State &state() const { return m_state; }
    void setState(const State &s) { m_state = s; }

private:
    int64_t m_warmup = 0;
    double m_decay = 1.0;
    int m_patience = 1;
    double m_min = 0.0, m_rate = 0.0;
    State m_state = {0, 1.0, 0, std::numeric_limits<double>::max()};
};

}  // namespace optimizers
}  // namespace currennt_hip
