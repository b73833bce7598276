// Stand-alone check of the group-width rule of the multi-column K_ff product (cglb_amd/csrc/pair_worklist.h), no HIP: prints, for every
// command line on stdin, what the library's launch code would do.
//   rule DH        -> "group partials(2) partials(4) partials(8)"
//   groups S GROUP -> the column counts of the groups a product of S columns is cut into, in order
#include <iostream>
#include <sstream>
#include <string>

#include "pair_worklist.h"

static_assert(MULTI_GROUP_NARROW == 8 && multi_group_pad(2) == 2 && multi_group_pad(3) == 4 && multi_group_pad(5) == 8 && multi_group_pad(8) == 8, "S_pad rule");

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "rule") {
            int dh = 0;
            in >> dh;
            std::cout << multi_mid_group(dh) << ' ' << multi_mid_partials(dh, 2) << ' ' << multi_mid_partials(dh, 4) << ' ' << multi_mid_partials(dh, 8) << '\n';
        } else if (cmd == "groups") {
            int s = 0, group = 0;
            in >> s >> group;
            if (group < 2 || s < 0) return 2;
            for (int b0 = 0, sg = 0; b0 < s; b0 += sg) {
                sg = multi_next_group(s - b0, group);
                if (sg < 1) return 3;
                std::cout << sg << ' ';
            }
            std::cout << '\n';
        } else {
            return 1;
        }
    }
    return 0;
}
