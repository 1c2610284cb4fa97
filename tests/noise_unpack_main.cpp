// Stand-alone check of lstm-rnn_amd/csrc/cn_noise_unpack.h (the host side of cn_dbg_noisy_weights), for a sanitizer build on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I lstm-rnn_amd/csrc tests/noise_unpack_main.cpp -o noise_unpack_check && ./noise_unpack_check
// Packs a flat weight vector into the layouts the pack kernels write (restated here, destination-indexed like them), gathers it
// back and compares; then plants a value in a pad entry of each copy and expects it to be counted.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cn_noise_unpack.h"

using namespace cn;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static void check_lstm(const UnitMap &prev, int dirs, int H, int Hp)
{
    const int P = prev.L, Pp = prev.Lp;
    NoiseUnpackGeom g{};
    g.lstm = 1; g.L = dirs * H; g.Lp = dirs * Hp; g.dirs = dirs; g.H = H; g.Hp = Hp;
    g.prev = prev;
    const long L = g.L, R = (long)dirs * 4 * Hp;
    const size_t nw = (size_t)(L * (4 * (P + 1) + 4 * H + 3));
    std::vector<float> w(nw);
    for (size_t k = 0; k < nw; ++k) w[k] = 1.0f + (float)k;
    std::vector<float> WinT((size_t)R * Pp, 0.f), WrecT((size_t)R * Hp, 0.f), peep((size_t)dirs * 3 * Hp, 0.f);
    for (long r = 0; r < R; ++r)
        for (int pc = 0; pc < Pp; ++pc) {
            const long d = r / (4 * Hp), j = (r / 4) % Hp, gg = r % 4;
            const int i = g.prev.unit(pc);
            if (j < H && i >= 0) WinT[(size_t)pc * R + r] = w[(size_t)(gg * L * P + d * H * P + j * P + i)];
        }
    for (long d = 0; d < dirs; ++d)
        for (long gg = 0; gg < 4; ++gg)
            for (long j = 0; j < H; ++j)
                for (long i = 0; i < H; ++i)
                    WrecT[(size_t)((d * Hp + i) * 4 * Hp + 4 * j + gg)] = w[(size_t)(4 * L * (P + 1) + gg * L * H + d * H * H + j * H + i)];
    for (long d = 0; d < dirs; ++d)
        for (long pp = 0; pp < 3; ++pp)
            for (long j = 0; j < H; ++j) peep[(size_t)((d * 3 + pp) * Hp + j)] = w[(size_t)(4 * L * (P + 1) + 4 * L * H + pp * L + d * H + j)];
    std::vector<float> flat(nw, -1.f);
    CHECK(noise_unpack(g, WinT, WrecT, peep, flat) == 0);
    const size_t b0 = (size_t)(4 * L * P), b1 = b0 + (size_t)(4 * L);
    for (size_t k = 0; k < nw; ++k) CHECK(flat[k] == ((k >= b0 && k < b1) ? -1.f : w[k]));       // the bias entries: untouched
    if (Hp > H) {
        std::vector<float> bad = WrecT; bad[(size_t)(H * 4 * Hp)] = 1e-30f;          // row i = H: a pad row
        CHECK(noise_unpack(g, WinT, bad, peep, flat) == 1);
        std::vector<float> badp = peep; badp[(size_t)H] = -1.f;
        CHECK(noise_unpack(g, WinT, WrecT, badp, flat) == 1);
        std::vector<float> badi = WinT; badi[(size_t)(4 * H)] = 2.f;                 // pc = 0, r = 4 * H: unit j = H of direction 0
        CHECK(noise_unpack(g, badi, WrecT, peep, flat) == 1);
    }
}

static void check_ff(const UnitMap &prev, int L, int Lp)
{
    const int P = prev.L, Pp = prev.Lp;
    NoiseUnpackGeom g{};
    g.lstm = 0; g.L = L; g.Lp = Lp; g.dirs = 1; g.prev = prev;
    const size_t nw = (size_t)L * (P + 1);
    std::vector<float> w(nw);
    for (size_t k = 0; k < nw; ++k) w[k] = 1.0f + (float)k;
    std::vector<float> WT((size_t)Pp * Lp, 0.f), none;
    for (int pc = 0; pc < Pp; ++pc) {
        const int i = g.prev.unit(pc);
        for (int j = 0; j < L; ++j) if (i >= 0) WT[(size_t)pc * Lp + j] = w[(size_t)j * P + i];
    }
    std::vector<float> flat(nw, -1.f);
    CHECK(noise_unpack(g, WT, none, none, flat) == 0);
    for (size_t k = 0; k < nw; ++k) CHECK(flat[k] == (k >= (size_t)L * P ? -1.f : w[k]));
    if (Lp > L) {
        std::vector<float> bad = WT; bad[(size_t)L] = 0.5f;
        CHECK(noise_unpack(g, bad, none, none, flat) == 1);
    }
}

int main()
{
    check_lstm({5, 8, 0, 0, 0}, 2, 6, 32);          // blstm 12 on a 5-wide input
    check_lstm({12, 64, 6, 32, 2}, 1, 7, 32);       // lstm 7 behind that blstm: columns of two padded directions
    check_lstm({3, 4, 0, 0, 0}, 1, 32, 32);         // no pad units
    check_ff({7, 32, 7, 32, 1}, 6, 32);             // feedforward 6 behind an lstm 7
    check_ff({6, 32, 0, 0, 0}, 4, 32);              // softmax 4 behind a dense layer
    std::printf(failures ? "noise_unpack: %d checks FAILED\n" : "noise_unpack: ok\n", failures);
    return failures ? 1 : 0;
}
