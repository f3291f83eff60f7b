// Host driver for pointrcnn_amd/csrc/level_units.h (tests/test_level_units_cpu.py): the workgroup -> (problem, local index, local
// count) table of the multi-problem launches.  Reads cases from stdin, one per line:
//     nprob cap  want[0..nprob)  weight[0..nprob)  units[0..nprob)        (weight -1 for all: no weights)
// and for every case deals the grid (level_units_share), walks EVERY workgroup of it (level_units_find) through a body that
// strides over its problem's units by its local count, and prints
//     grid  g[0..nprob)  ok
// ok = 1 when every unit of every problem was visited exactly once, no workgroup fell outside its problem, the shares respect
// want / cap and no problem that wants workgroups was left without one.  A refused case prints "-1".
#include <cstdio>
#include <vector>
#include "level_units.h"

int main() {
    int nprob;
    long cap;
    while (scanf("%d %ld", &nprob, &cap) == 2) {
        long want[LEVEL_MAX_PROBLEMS] = {0, 0, 0, 0}, weight[LEVEL_MAX_PROBLEMS] = {0, 0, 0, 0}, units[LEVEL_MAX_PROBLEMS] = {0, 0, 0, 0};
        if (nprob < 0 || nprob > LEVEL_MAX_PROBLEMS) {
            long skip;
            for (int i = 0; i < 3 * nprob; i++) if (scanf("%ld", &skip) != 1) return 2;
            LevelUnits U = {};
            printf("%ld\n", level_units_share(U, want, nullptr, nprob, cap));
            continue;
        }
        for (int p = 0; p < nprob; p++) if (scanf("%ld", &want[p]) != 1) return 2;
        for (int p = 0; p < nprob; p++) if (scanf("%ld", &weight[p]) != 1) return 2;
        for (int p = 0; p < nprob; p++) if (scanf("%ld", &units[p]) != 1) return 2;
        bool weighted = false;
        for (int p = 0; p < nprob; p++) weighted = weighted || weight[p] >= 0;
        LevelUnits U = {};
        const long grid = level_units_share(U, want, weighted ? weight : nullptr, nprob, cap);
        if (grid < 0) { printf("-1\n"); continue; }
        bool ok = U.nprob == nprob && (nprob == 0 || U.end[nprob - 1] == grid);
        long sum_want = 0, g[LEVEL_MAX_PROBLEMS];
        for (int p = 0; p < nprob; p++) {
            g[p] = U.end[p] - (p ? U.end[p - 1] : 0);
            sum_want += want[p];
            ok = ok && g[p] >= 0 && g[p] <= want[p] && (want[p] == 0 || g[p] >= 1);
        }
        ok = ok && (cap <= 0 || sum_want <= cap ? grid == sum_want : grid == cap);
        std::vector<std::vector<int>> seen(nprob);
        for (int p = 0; p < nprob; p++) seen[p].assign((size_t)units[p], 0);
        for (long b = 0; b < grid; b++) {
            int prob = -1, local = -1, count = -1;
            level_units_find(U, (int)b, prob, local, count);
            if (prob < 0 || prob >= nprob || count != g[prob] || local < 0 || local >= count) { ok = false; continue; }
            for (long u = local; u < units[prob]; u += count) seen[prob][(size_t)u]++;
        }
        for (int p = 0; p < nprob; p++)
            for (long u = 0; u < units[p]; u++) ok = ok && (seen[p][(size_t)u] == 1 || (want[p] == 0 && seen[p][(size_t)u] == 0));
        printf("%ld", grid);
        for (int p = 0; p < nprob; p++) printf(" %ld", g[p]);
        printf(" %d\n", ok ? 1 : 0);
    }
    return 0;
}
