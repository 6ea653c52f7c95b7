// The lane -> LDS maps of the wide conv form's row-major epilogue (aware_amd/csrc/conv_epilogue_rows.hpp) walked on the CPU:
// no HIP header, no GPU.  For RG = 1, 2, 3 and each of the four maps (c_write, c_read, act_write, act_read) one line
//   RG r map name bijection b owner o ways64 w wayshw h
// bijection  1 when the map's (lane, register) pairs cover every float of the wave's region exactly once;
// owner      1 when the map sends the element (row, col) that a lane's register holds in one layout to the slot from which
//            the other layout's map reads that same (row, col): the turn returns every element to its owner;
// ways64     worst wave instruction of the map on 64 banks of 4 bytes, all 64 lanes counted together: the largest number of
//            distinct words on one bank, over the least that many words can have (64 lanes x 1 word: 1; x 4 words: 4);
// wayshw     the same per lane group and bank count of the instruction as the hardware serves it: 4-byte accesses in two
//            halves of 32 lanes on 32 banks, ds_read_b128 in four groups of 16 lanes on 64 banks, ds_write_b128 in eight
//            groups of 8 consecutive lanes on 32 banks.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../aware_amd/csrc/conv_epilogue_rows.hpp"

namespace er = aware::epi_rows;

struct Access { int lane, word, nwords; };        // one lane's access of one wave instruction (float index, 1 or 4 floats)

// largest number of distinct words on one bank among the lanes of `group`, over the least possible for that many words
static double ways(const std::vector<Access>& ins, const std::vector<int>& group, int banks) {
    std::map<int, std::set<int>> on_bank;
    std::set<int> words;
    for (const Access& a : ins) {
        if (std::find(group.begin(), group.end(), a.lane) == group.end()) continue;
        for (int k = 0; k < a.nwords; ++k) { on_bank[(a.word + k) % banks].insert(a.word + k); words.insert(a.word + k); }
    }
    size_t worst = 0;
    for (auto& b : on_bank) worst = std::max(worst, b.second.size());
    const size_t least = (words.size() + banks - 1) / banks;
    return (double)worst / (double)least;
}

static std::vector<std::vector<int>> lane_groups(const char* kind) {
    std::vector<std::vector<int>> g;
    const std::string k = kind;
    if (k == "b32") {
        g.resize(2);
        for (int l = 0; l < 64; ++l) g[l >> 5].push_back(l);
    } else if (k == "read_b128") {
        // {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same in the upper half
        g.resize(4);
        for (int l = 0; l < 64; ++l) {
            const int q = l & 31;
            const bool first = q < 4 || (q >= 12 && q < 16) || (q >= 20 && q < 28);
            g[2 * (l >> 5) + (first ? 0 : 1)].push_back(l);
        }
    } else {
        g.resize(8);
        for (int l = 0; l < 64; ++l) g[l >> 3].push_back(l);
    }
    return g;
}

int main() {
    std::vector<int> all(64);
    for (int l = 0; l < 64; ++l) all[l] = l;
    for (int RG = 1; RG <= 3; ++RG) {
        const int MT = 2 * RG, RJ = er::row_passes(RG), NF = er::region_floats(RG);
        struct Map { const char* name; bool acc; const char* kind; int banks_hw; };
        const Map maps[4] = {{"c_write", true, "b32", 32}, {"c_read", false, "read_b128", 64},
                             {"act_write", false, "write_b128", 32}, {"act_read", true, "b32", 32}};
        for (const Map& mp : maps) {
            // the map's wave instructions, and the (row, col) each slot holds according to the map's own layout
            std::vector<std::vector<Access>> instr;
            std::vector<int> hits(NF, 0), holds(NF, -1);
            if (mp.acc) {
                for (int m = 0; m < MT; ++m)
                    for (int nl = 0; nl < 2; ++nl)
                        for (int e = 0; e < 4; ++e) {
                            std::vector<Access> in;
                            for (int lane = 0; lane < 64; ++lane) {
                                const int w = mp.name[0] == 'c' ? er::c_write(lane, m, nl, e) : er::act_read(lane, m, nl, e);
                                in.push_back({lane, w, 1});
                                if (w >= 0 && w < NF) { ++hits[w]; holds[w] = er::acc_row(lane, m, e) * er::kCols + er::acc_col(lane, nl); }
                            }
                            instr.push_back(in);
                        }
            } else {
                for (int j = 0; j < RJ; ++j) {
                    std::vector<Access> in;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int w = mp.name[0] == 'c' ? er::c_read(lane, j) : er::act_write(lane, j);
                        in.push_back({lane, w, 4});
                        for (int k = 0; k < 4; ++k)
                            if (w + k >= 0 && w + k < NF) {
                                ++hits[w + k];
                                holds[w + k] = er::rm_row(lane, j) * er::kCols + er::rm_col(lane) + k;
                            }
                    }
                    instr.push_back(in);
                }
            }
            bool bij = true;
            for (int i = 0; i < NF; ++i) bij = bij && hits[i] == 1;
            for (auto& in : instr)
                for (const Access& a : in) bij = bij && a.word >= 0 && a.word + a.nwords <= NF && (a.nwords == 1 || a.word % 4 == 0);
            // the other layout's view of every slot: both must name the same (row, col)
            bool owner = true;
            std::vector<int> other(NF, -2);
            if (mp.acc) {
                for (int j = 0; j < RJ; ++j)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int k = 0; k < 4; ++k) {
                            const int w = (mp.name[0] == 'c' ? er::c_read(lane, j) : er::act_write(lane, j)) + k;
                            if (w >= 0 && w < NF) other[w] = er::rm_row(lane, j) * er::kCols + er::rm_col(lane) + k;
                        }
            } else {
                for (int m = 0; m < MT; ++m)
                    for (int nl = 0; nl < 2; ++nl)
                        for (int e = 0; e < 4; ++e)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int w = mp.name[0] == 'c' ? er::c_write(lane, m, nl, e) : er::act_read(lane, m, nl, e);
                                if (w >= 0 && w < NF) other[w] = er::acc_row(lane, m, e) * er::kCols + er::acc_col(lane, nl);
                            }
            }
            for (int i = 0; i < NF; ++i) owner = owner && holds[i] == other[i];
            double w64 = 0, whw = 0;
            const auto groups = lane_groups(mp.kind);
            for (auto& in : instr) {
                w64 = std::max(w64, ways(in, all, 64));
                for (auto& g : groups) whw = std::max(whw, ways(in, g, mp.banks_hw));
            }
            std::printf("RG %d map %s bijection %d owner %d ways64 %g wayshw %g\n", RG, mp.name, (int)bij, (int)owner, w64, whw);
        }
    }
    return 0;
}
