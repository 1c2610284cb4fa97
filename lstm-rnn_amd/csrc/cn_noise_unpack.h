// Host side of cn_dbg_noisy_weights: gathers the noisy operand copies of one layer (already widened to float, in the packed
// layouts lstm_pack_body / ff_pack_body write) back into the flat reference layout, and checks that every pad entry is exactly
// zero.  Plain C++, no device code: csrc/cn_api.cpp includes it, and tests/noise_unpack_main.cpp builds it stand-alone.
#pragma once

#include <stddef.h>
#include <vector>

#include "cn_unit_map.h"

namespace cn {

struct NoiseUnpackGeom {
    int lstm;                             // 1: LSTM layer (dirs, H, Hp used), 0: dense layer (L, Lp used)
    int L, Lp;                            // layer size; dense layers: padded width
    int dirs, H, Hp;
    UnitMap prev;                         // the preceding layer's rows: the columns of WinT's rows
};

// WinT: LSTM [Pp][dirs*4*Hp] (row r = (d*Hp + j)*4 + gate), dense [Pp][Lp]; WrecT: [dirs][Hp][4*Hp] (k = 4*j + gate contiguous);
// peep: [dirs][3][Hp].  flat: the layer's weight vector, whose entries with a noisy counterpart are overwritten (the bias entries
// stay what the caller put there).  Returns the number of pad entries that are not exactly zero.
inline size_t noise_unpack(const NoiseUnpackGeom &g, const std::vector<float> &WinT, const std::vector<float> &WrecT,
                           const std::vector<float> &peep, std::vector<float> &flat)
{
    size_t bad = 0;
    const long P = g.prev.L, L = g.L;
    if (!g.lstm) {
        for (int pc = 0; pc < g.prev.Lp; ++pc) {
            const int i = g.prev.unit(pc);
            for (int j = 0; j < g.Lp; ++j) {
                const float v = WinT[(size_t)pc * g.Lp + j];
                if (j < g.L && i >= 0) flat[(size_t)j * P + i] = v;
                else if (v != 0.f || v != v) ++bad;
            }
        }
        return bad;
    }
    const long H = g.H, Hp = g.Hp, R = (long)g.dirs * 4 * Hp;
    for (int pc = 0; pc < g.prev.Lp; ++pc) {
        const int i = g.prev.unit(pc);
        for (long r = 0; r < R; ++r) {
            const long d = r / (4 * Hp), j = (r / 4) % Hp, gg = r % 4;
            const float v = WinT[(size_t)pc * R + r];
            if (j < H && i >= 0) flat[(size_t)(gg * L * P + d * H * P + j * P + i)] = v;
            else if (v != 0.f || v != v) ++bad;
        }
    }
    for (long d = 0; d < g.dirs; ++d)
        for (long i = 0; i < Hp; ++i)
            for (long k = 0; k < 4 * Hp; ++k) {
                const long j = k / 4, gg = k % 4;
                const float v = WrecT[(size_t)((d * Hp + i) * 4 * Hp + k)];
                if (j < H && i < H) flat[(size_t)(4 * L * (P + 1) + gg * L * H + d * H * H + j * H + i)] = v;
                else if (v != 0.f || v != v) ++bad;
            }
    for (long d = 0; d < g.dirs; ++d)
        for (long pp = 0; pp < 3; ++pp)
            for (long j = 0; j < Hp; ++j) {
                const float v = peep[(size_t)((d * 3 + pp) * Hp + j)];
                if (j < H) flat[(size_t)(4 * L * (P + 1) + 4 * L * H + pp * L + d * H + j)] = v;
                else if (v != 0.f || v != v) ++bad;
            }
    return bad;
}

}  // namespace cn
