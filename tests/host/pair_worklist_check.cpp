// Stand-alone driver of cglb_amd/csrc/pair_worklist.h for tests/test_pair_worklist_host.py (no HIP, no GPU).
// Reads commands from standard input, one per line, and answers each with one line:
//   chunk N RBROWS WORLD OPT                     -> pair_column_chunk
//   order NGROUPS NUNITS ORDER F_0 ... F_{NGROUPS-1}  -> the (group, unit) pairs of pair_work_order with first_unit(g) = F_g: "g k g k ..."
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "pair_worklist.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "chunk") {
            long long n, opt;
            int rbrows, world;
            if (!(in >> n >> rbrows >> world >> opt)) return 2;
            std::printf("%lld\n", (long long)pair_column_chunk(n, rbrows, world, opt));
        } else if (cmd == "order") {
            int ngroups, nunits, order;
            if (!(in >> ngroups >> nunits >> order)) return 2;
            std::vector<int> first(ngroups);
            for (int& f : first)
                if (!(in >> f)) return 2;
            const std::vector<pair_unit> list = pair_work_order(ngroups, nunits, [&](int g) { return first[g]; }, order);
            for (const pair_unit& u : list) std::printf("%d %d ", u.x, u.y);
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
