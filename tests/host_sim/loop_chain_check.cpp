// The embed loop's chain parser and workspace carver (aware_amd/csrc/loop_chain.hpp) on the CPU: no HIP header, no GPU.
// stdin:  dims B NS NF pstride out_len[0..B)          the batch every later case is parsed against
//         chain N ex | N lines "kind prob p0 p1 p2 p3"  -> "rc bytes": parse_loop_chain's return code (ex = 0: the older
//                                                         entry points) and loop_chain_workspace_bytes
//         mixture M | M times: "weight N" and N entry lines -> "rc bytes": parse_loop_mixture, loop_mixture_workspace_bytes
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../aware_amd/csrc/loop_chain.hpp"

using namespace aware;

// a float as strtof reads it: nan and inf included, which operator>> refuses
static float read_float() {
    std::string tok;
    std::cin >> tok;
    return strtof(tok.c_str(), nullptr);
}
static std::vector<aware_loop_attack_ex> read_entries(int n) {
    std::vector<aware_loop_attack_ex> v(n);
    for (auto& a : v) {
        std::cin >> a.kind;
        a.prob = read_float();
        for (float& p : a.param) p = read_float();
    }
    return v;
}

int main() {
    LoopDims d;
    std::vector<int> out_len;
    std::string word;
    while (std::cin >> word) {
        if (word == "dims") {
            std::cin >> d.B >> d.NS >> d.NF >> d.pstride;
            out_len.assign(d.B, 0);
            for (int& n : out_len) std::cin >> n;
            d.out_len = out_len.data();
        } else if (word == "chain") {
            int n, ex;
            std::cin >> n >> ex;
            const std::vector<aware_loop_attack_ex> ent = read_entries(n);
            LoopChainState la;
            const int rc = parse_loop_chain(d, ent.data(), n, ex != 0, la);
            printf("%d %zu\n", rc, loop_chain_workspace_bytes(d, ent.data(), n));
        } else if (word == "mixture") {
            int m;
            std::cin >> m;
            std::vector<std::vector<aware_loop_attack_ex>> ent(m);
            std::vector<aware_loop_chain> chains(m);
            for (int c = 0; c < m; ++c) {
                int n;
                chains[c].weight = read_float();
                std::cin >> n;
                ent[c] = read_entries(n);
                chains[c].attacks = ent[c].data(); chains[c].n_attacks = n;
            }
            LoopChainState mix[kMaxLoopChains];
            unsigned long long thr[kMaxLoopChains];
            int rv = -1;
            const int rc = parse_loop_mixture(d, chains.data(), m, mix, thr, rv);
            printf("%d %zu\n", rc, loop_mixture_workspace_bytes(d, chains.data(), m));
        } else {
            fprintf(stderr, "unknown word %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
