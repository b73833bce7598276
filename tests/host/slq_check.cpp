// Stand-alone driver of cglb_amd/csrc/slq_host.h for tests/test_slq_host.py (no HIP).  One command per input line, one output line each:
//   quad n d_0 .. d_{n-1} e_0 .. e_{n-2}      -> "<status> <e_1^T log(T) e_1>"
//   steps S t col L rz[(S+1)(1+t)] pap[S(1+t)] -> "<usable steps of column col>"
//   tri S t col J rz[...] pap[...]             -> "d_0 .. d_{J-1} e_0 .. e_{J-1}"
//   corr S t L rz[...] pap[...]                -> "<status> <(1/t) sum_i rz_0i e_1^T log(T_i) e_1>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "slq_host.h"

static double number(std::istringstream& in) {
    std::string tok;
    if (!(in >> tok)) { std::fprintf(stderr, "short command\n"); std::exit(2); }
    return std::strtod(tok.c_str(), nullptr);  // reads "nan" and "inf" as well
}

static void logs(std::istringstream& in, int S, int t, std::vector<double>& rz, std::vector<double>& pap) {
    rz.resize((size_t)(S + 1) * (1 + t));
    pap.resize((size_t)S * (1 + t));
    for (double& v : rz) v = number(in);
    for (double& v : pap) v = number(in);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        std::vector<double> rz, pap;
        if (cmd == "quad") {
            const int n = (int)number(in);
            std::vector<double> d((size_t)n), e((size_t)n, 0.0);
            for (int i = 0; i < n; ++i) d[i] = number(in);
            for (int i = 0; i + 1 < n; ++i) e[i] = number(in);
            int st = -1;
            const double v = slq_e1_log_e1(d, e, &st);
            std::printf("%d %.17g\n", st, v);
        } else if (cmd == "steps") {
            const int S = (int)number(in), t = (int)number(in), col = (int)number(in), L = (int)number(in);
            logs(in, S, t, rz, pap);
            std::printf("%d\n", slq_usable_steps(rz.data(), pap.data(), S, 1 + t, col, L));
        } else if (cmd == "tri") {
            const int S = (int)number(in), t = (int)number(in), col = (int)number(in), J = (int)number(in);
            logs(in, S, t, rz, pap);
            std::vector<double> d, e;
            slq_tridiagonal(rz.data(), pap.data(), 1 + t, col, J, d, e);
            for (int i = 0; i < J; ++i) std::printf("%.17g ", d[i]);
            for (int i = 0; i < J; ++i) std::printf("%.17g%s", e[i], i + 1 < J ? " " : "");
            std::printf("\n");
        } else if (cmd == "corr") {
            const int S = (int)number(in), t = (int)number(in), L = (int)number(in);
            logs(in, S, t, rz, pap);
            int st = -1;
            const double v = slq_logdet_correction(rz.data(), pap.data(), S, t, L, &st);
            std::printf("%d %.17g\n", st, v);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
