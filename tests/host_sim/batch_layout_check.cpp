// csrc/batch_layout.hpp on the CPU (no HIP): reads one batch per line,
//   card <B> <has_offsets> n_0 .. n_{B-1} [off_0 .. off_{B-1}]
//   gen <n_fft> <hop> <B> <has_offsets> n_0 .. [off_0 ..]
// and prints one JSON object per line: rc (0, or -1 where the constructors refuse), the scalars and every table, composed as
// aware_batch_create / aware_batch_create_for_plan compose them.  Run by tests/test_batch_layout_host.py.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../../aware_amd/csrc/batch_layout.hpp"

using namespace aware;

// the card's constants as fft512.hpp, kernels.h and common.hpp define them (those headers need HIP)
constexpr int kHop = 256, kHalf = 512, kStreamWaves = 4, kSynthBlocks = 16;

static void tab(const char* name, const std::vector<int>& v) {
    printf(", \"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf(i ? ",%d" : "%d", v[i]);
    printf("]");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string route;
        if (!(in >> route)) continue;
        const bool gen = route == "gen";
        int n_fft = 2 * kHalf, hop = kHop, B = 0, has_off = 0;
        if (gen) in >> n_fft >> hop;
        in >> B >> has_off;
        std::vector<int> n(B), off(B);
        for (int& v : n) in >> v;
        if (has_off)
            for (int& v : off) in >> v;
        BatchLayout L;
        if (!in || B < 1 || !batch_layout(n.data(), has_off ? off.data() : nullptr, B, hop, n_fft / 2, L)) {
            printf("{\"rc\": -1}\n");
            continue;
        }
        CardRuns C;
        if (!gen) card_runs(n.data(), hop, kStreamWaves, kSynthBlocks, L, C);
        printf("{\"rc\": 0, \"NF\": %d, \"NP\": %d, \"NS\": %d, \"max_frames\": %d, \"max_len\": %d, \"pstride\": %d, \"uniform_tp\": %d",
               L.NF, L.NP, L.NS, L.max_frames, L.max_len, L.pstride, L.uniform_tp);
        tab("in_off", L.in_off); tab("T", L.T); tab("frame_off", L.frame_off); tab("pool_off", L.pool_off);
        tab("out_off", L.out_off); tab("out_len", L.out_len); tab("pc_in", L.pc_in); tab("order", L.order);
        if (gen) {
            tab("pc_out", pc_out_for(L.out_len));
        } else {
            printf(", \"synth_run\": %d, \"an_run\": %d, \"n_an_wg\": %d, \"n_syn_wg\": %d", C.synth_run, C.an_run,
                   (int)C.an_wg.size(), (int)C.syn_wg.size());
            tab("pc_syn", C.pc_syn); tab("an_wg", C.an_wg); tab("syn_wg", C.syn_wg);
        }
        printf("}\n");
    }
    return 0;
}
