// Stand-alone driver of cglb_amd/csrc/lanczos_host.h for tests/test_love_ref_host.py (no HIP).  One command per input line, one output line each:
//   factor J a_0 .. a_{J-1} b_0 .. b_{J-2}  -> "<status> d_0 .. d_{J-1} l_0 .. l_{J-1}"
//   stop j rank beta alpha0                 -> "0" or "1"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lanczos_host.h"

static double number(std::istringstream& in) {
    std::string tok;
    if (!(in >> tok)) { std::fprintf(stderr, "short command\n"); std::exit(2); }
    return std::strtod(tok.c_str(), nullptr);  // reads "nan" and "inf" as well
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "factor") {
            const int J = (int)number(in);
            std::vector<double> a((size_t)J), b((size_t)(J > 1 ? J - 1 : 0)), d, l;
            for (double& v : a) v = number(in);
            for (double& v : b) v = number(in);
            const int st = lanczos_bidiag_factor(a.data(), b.data(), J, d, l);
            std::printf("%d", st);
            for (double v : d) std::printf(" %.17g", v);
            for (double v : l) std::printf(" %.17g", v);
            std::printf("\n");
        } else if (cmd == "stop") {
            const int j = (int)number(in), rank = (int)number(in);
            const double beta = number(in), alpha0 = number(in);
            std::printf("%d\n", lanczos_stop(j, rank, beta, alpha0) ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
