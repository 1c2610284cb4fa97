// Stand-alone check of lstm-rnn_amd/csrc/cn_unit_map.h, the one statement of where a layer's units lie in its padded rows, built
// with the host C++ compiler (tests/test_unit_map_host.py), or by hand for a sanitizer build on the CPU:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I lstm-rnn_amd/csrc tests/unit_map_main.cpp -o unit_map_check && ./unit_map_check
// Walks dense, one-directional and two-directional maps and holds col / unit / units_in_group to a brute-force restatement:
// a table of the unit of every column, filled from the layout's definition alone.
#include <cstdio>
#include <vector>

#include "cn_unit_map.h"

using namespace cn;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, what); ++failures; } } while (0)

static int round_up(int x, int m) { return (x + m - 1) / m * m; }

static void walk(const char *what, const UnitMap &m)
{
    // the definition: unit u of a dense row at column u; direction d's unit j, unit d * H + j, at column d * Hp + j
    std::vector<int> unit_of(m.Lp, -1);
    if (m.H == 0) for (int u = 0; u < m.L; ++u) unit_of[u] = u;
    else
        for (int d = 0; d < m.dirs; ++d)
            for (int j = 0; j < m.H; ++j) unit_of[d * m.Hp + j] = d * m.H + j;
    int prev_col = -1;
    for (int u = 0; u < m.L; ++u) {
        const int c = m.col(u);
        CHECK(c >= 0 && c < m.Lp);
        if (c < 0 || c >= m.Lp) continue;
        CHECK(unit_of[c] == u);
        CHECK(m.unit(c) == u);                           // unit(col(u)) == u
        CHECK(c > prev_col);                             // strictly ascending
        prev_col = c;
    }
    for (int c = 0; c < m.Lp; ++c) CHECK(m.unit(c) == unit_of[c]);       // every column that is no unit's column: -1
    for (int G = 4; G <= 8; G += 4)
        for (int c = 0; c < m.Lp; c += G) {
            int brute = 0;
            for (int k = 0; k < G && c + k < m.Lp; ++k) brute += unit_of[c + k] >= 0;
            const int cnt = m.units_in_group(c, G);
            CHECK(cnt == brute);
            for (int k = 0; k < G && c + k < m.Lp; ++k) CHECK((unit_of[c + k] >= 0) == (k < cnt));     // the units come first
        }
}

int main()
{
    const int dense[] = {1, 5, 32, 33};
    for (int L : dense) walk("dense", UnitMap{L, round_up(L, 32), 0, 0, 0});
    walk("one direction, H = 7", UnitMap{7, 32, 7, 32, 1});
    walk("one direction, H = 32", UnitMap{32, 32, 32, 32, 1});
    const int two[] = {5, 6, 32};
    for (int H : two) walk("two directions, Hp = 32", UnitMap{2 * H, 64, H, 32, 2});
    walk("two directions of 125", UnitMap{250, 256, 125, 128, 2});
    walk("two directions of 520", UnitMap{1040, 1152, 520, 576, 2});
    std::printf(failures ? "unit_map: %d checks FAILED\n" : "unit_map: ok\n", failures);
    return failures ? 1 : 0;
}
