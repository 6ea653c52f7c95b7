// Host model of the LDS banking of the wave-level FFT in aware_amd/csrc/fft512.hpp: every exchange and table access of one
// frame is evaluated for lanes 0..63 with the index functions the device phases use, under the rule of the instruction that
// moves it (lane groups that are served together, bank of a 4-byte word):
//     ds_read_b64    two groups of 32 consecutive lanes,   word mod 64
//     ds_write_b64   four groups of 16 consecutive lanes,  word mod 32   (ds_write2_b64: two such accesses)
//     ds_read2_b64   per access four groups of 16 lanes,   word mod 32   (the former pairing of the loads: shown, not asserted)
// Lanes of a group that name the same address share one access; every further distinct address on a busy bank costs the
// group one more cycle.  An 8-byte access takes an even / odd pair of banks, so in cf units the bank is index mod 32 (reads)
// or index mod 16 (the mod-32 rule).
// Also checked on the index functions: each exchange is the transpose tests/host_sim/fft_sim.cpp verifies numerically (the
// element a load names is the one the matching store put there), is injective and stays inside kFftScratch.
// Built and run by tests/test_fft_lds_banks_host.py.  Not modelled: the mel rows (their offsets are the filter bank's, data)
// and ds_bpermute_b32 (no LDS memory).
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>
#include "../../aware_amd/csrc/fft512.hpp"

using namespace aware;

struct Rule {
    const char* name;
    int group;      // consecutive lanes served together
    int mod_cf;     // banks / 2: two 8-byte accesses conflict when their cf indices agree mod this
    int base;       // LDS cycles of the conflict-free wave instruction (one per group)
};
static const Rule kRead64 = {"ds_read_b64", 32, 32, 2};
static const Rule kWrite64 = {"ds_write_b64", 16, 16, 4};
static const Rule kRead2x64 = {"ds_read2_b64", 16, 16, 4};      // per access of the pair

// extra cycles of one wave access: per group, (largest number of distinct addresses on one bank) - 1
template <class F> static int conflicts(const Rule& r, F index) {
    int extra = 0;
    for (int g = 0; g < 64; g += r.group) {
        std::vector<std::set<int>> bank(r.mod_cf);
        for (int l = g; l < g + r.group; ++l) bank[index(l) % r.mod_cf].insert(index(l));
        size_t worst = 1;
        for (auto& b : bank) worst = b.size() > worst ? b.size() : worst;
        extra += (int)worst - 1;
    }
    return extra;
}

static int total_bad = 0;
// one row: `what` is 8 (or 7) wave accesses, one per register
template <class F> static void row(const char* what, const Rule& r, int r0, int r1, F index, bool asserted) {
    int extra = 0, cycles = 0;
    for (int reg = r0; reg < r1; ++reg) {
        extra += conflicts(r, [&](int l) { return index(l, reg); });
        cycles += r.base;
    }
    printf("%-28s %-13s accesses %d cycles %d conflict_cycles %d%s\n", what, r.name, r1 - r0, cycles + extra, extra,
           asserted ? "" : " (former layout)");
    if (asserted) total_bad += extra;
}

int main() {
    // ---- this tree ----
    row("xch1_store", kWrite64, 0, 8, [](int l, int k0) { return xch1_store_index(l, k0); }, true);
    row("xch1_load", kRead64, 0, 8, [](int l, int n1) { return xch1_load_index(l, n1); }, true);
    row("xch2_store", kWrite64, 0, 8, [](int l, int q0) { return xch2_store_index(l, q0); }, true);
    row("xch2_load", kRead64, 0, 8, [](int l, int n0) { return xch2_load_index(l, n0); }, true);
    row("tw1s", kRead64, 1, 8, [](int l, int k0) { return k0 * 64 + l; }, true);
    row("tw2s", kRead64, 1, 8, [](int l, int q0) { return tw2_index(l, q0); }, true);
    row("wins / mcs", kRead64, 0, 8, [](int l, int r) { return l + 64 * r; }, true);
    // ---- the layouts and pairings this replaced (k0*73 + 8*q0 + n0, tw2s[n0*8 + q0], paired loads) ----
    row("old xch2_store", kWrite64, 0, 8, [](int l, int q0) { return (l >> 3) * 73 + 8 * q0 + (l & 7); }, false);
    row("old xch2_load", kRead2x64, 0, 8, [](int l, int n0) { return (l & 7) * 73 + 8 * (l >> 3) + n0; }, false);
    row("old xch1_load", kRead2x64, 0, 8, [](int l, int n1) { return (l >> 3) * 72 + 8 * n1 + (l & 7); }, false);
    row("old tw1s", kRead2x64, 1, 8, [](int l, int k0) { return k0 * 64 + l; }, false);
    row("old tw2s", kRead2x64, 1, 8, [](int l, int q0) { return (l & 7) * 8 + q0; }, false);
    row("old tw2s as ds_read_b64", kRead64, 1, 8, [](int l, int q0) { return (l & 7) * 8 + q0; }, false);
    row("old wins / mcs", kRead2x64, 0, 8, [](int l, int r) { return l + 64 * r; }, false);

    // ---- the exchanges are the transposes of fft_sim.cpp ----
    int perm_bad = 0;
    std::set<int> used1, used2;
    for (int l = 0; l < 64; ++l)
        for (int r = 0; r < 8; ++r) {
            // exchange 1: lane (k0, n0) register n1 takes element 8*n1 + n0 of row k0, stored by lane 8*n1 + n0 from register k0
            if (xch1_load_index(l, r) != xch1_store_index(8 * r + (l & 7), l >> 3)) ++perm_bad;
            // exchange 2: lane (k0 = l & 7, q0 = l >> 3) register n0 takes (k0, q0, n0), stored by lane 8*k0 + n0 from register q0
            if (xch2_load_index(l, r) != xch2_store_index(8 * (l & 7) + r, l >> 3)) ++perm_bad;
            used1.insert(xch1_store_index(l, r));
            used2.insert(xch2_store_index(l, r));
            for (int i : {xch1_store_index(l, r), xch2_store_index(l, r), xch1_load_index(l, r), xch2_load_index(l, r)})
                if (i < 0 || i >= kFftScratch) ++perm_bad;
        }
    if (used1.size() != 512 || used2.size() != 512) ++perm_bad;
    // the twiddle table is symmetric, so [q0][n0] reads what [n0][q0] read
    cf tw512[512], t1[512], t2[64];
    for (int j = 0; j < 512; ++j) tw512[j] = mk((float)j, (float)-j);      // distinct tags, not twiddles
    for (int tid = 0; tid < 256; ++tid) fft_fill_tables(tid, 256, tw512, t1, t2);
    for (int l = 0; l < 64; ++l)
        for (int q0 = 1; q0 < 8; ++q0)
            if (std::memcmp(&t2[tw2_index(l, q0)], &t2[(l & 7) * 8 + q0], sizeof(cf)) != 0) ++perm_bad;
    printf("permutation_errors %d\n", perm_bad);
    printf("asserted_conflict_cycles %d\n", total_bad);
    return (perm_bad || total_bad) ? 1 : 0;
}
