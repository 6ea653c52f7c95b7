// The general route's chain parser and workspace carver (aware_amd/csrc/loop_any_chain.hpp) on the CPU: no HIP header, no GPU.
// stdin:  dims B NS NF pstride out_len[0..B)          the batch every later case is parsed against
//         chain N | N lines "kind prob p0 p1 p2 p3"  -> "rc bytes": parse_gen_chain's return code (what
//                                                       aware_embed_set_general_chain returns for a general session before it
//                                                       looks at the workspace) and gen_chain_workspace_bytes
// The workspace check itself: "carve BYTES" -> "ok pieces": whether a workspace of BYTES holds the carve of the last chain
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../aware_amd/csrc/loop_any_chain.hpp"

using namespace aware;

// a float as strtof reads it: nan and inf included, which operator>> refuses
static float read_float() {
    std::string tok;
    std::cin >> tok;
    return strtof(tok.c_str(), nullptr);
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
            int n;
            std::cin >> n;
            std::vector<aware_loop_attack_ex> ent(n);
            for (auto& a : ent) {
                std::cin >> a.kind;
                a.prob = read_float();
                for (float& p : a.param) p = read_float();
            }
            GenChainState g;
            const int rc = parse_gen_chain(d, n ? ent.data() : nullptr, n, g);
            printf("%d %zu\n", rc, gen_chain_workspace_bytes(d, n ? ent.data() : nullptr, n));
        } else if (word == "carve") {
            size_t bytes;
            std::cin >> bytes;
            GenChainState g;
            Carver c((void*)256, bytes);
            carve_gen_chain(c, d, g);
            printf("%d %d\n", c.ok ? 1 : 0, g.pieces);
        } else {
            fprintf(stderr, "unknown word %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
