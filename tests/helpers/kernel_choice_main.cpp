// Replays every row of a kernel-choice table (tools/kernel_choice_table.py; tests/golden/kernel_choice_256cu.json) through
// choose_cov / choose_pow of csrc/kernel_choice.h with the row's recorded occupancy figures and CU count, and checks the traits'
// own invariants on each row.  Plain C++: no GPU, no HIP.  Prints "kernel choice ok: N rows" or the rows that differ.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "kernel_choice.h"

using namespace oiva;

namespace {
enum { cT, cF, cFtot, cM, cK, cPrec, cQuad, cHm, cCovReq, cPowReq, cPart32, cKind, cNsplit, cTc, cKc, cNbg, cPad, cP32, cV64, cUnit, cPow,
       cNb, cPns, cTcp, cKp, cRounds, cOccCov, cOccPow, cNcu, kCols };

std::vector<std::vector<int>> read_rows(const char* path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    std::vector<std::vector<int>> rows;
    size_t i = s.find("\"rows\":[");
    if (i == std::string::npos) return rows;
    i += 8;
    while ((i = s.find('[', i)) != std::string::npos) {
        const size_t e = s.find(']', i);
        std::vector<int> r;
        std::stringstream line(s.substr(i + 1, e - i - 1));
        for (std::string tok; std::getline(line, tok, ',');) r.push_back(std::stoi(tok));
        rows.push_back(r);
        i = e + 1;
    }
    return rows;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const auto rows = read_rows(argv[1]);
    if (rows.empty()) {
        std::printf("no rows in %s\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (size_t n = 0; n < rows.size(); ++n) {
        const std::vector<int>& r = rows[n];
        if ((int)r.size() != kCols) {
            std::printf("row %zu: %zu columns\n", n, r.size());
            return 2;
        }
        ChoiceIn c{};
        c.T = r[cT], c.F = r[cF], c.F_total = r[cFtot], c.M = r[cM], c.K = r[cK], c.n_cu = r[cNcu];
        c.cov_f64 = r[cPrec] & OIVA_PREC_COV_F64, c.upd_f64 = r[cPrec] & OIVA_PREC_UPDATE_F64;
        c.cov_quad_on = r[cQuad], c.cov_hmfma_on = r[cHm], c.part32 = r[cPart32];
        int asked[2] = {-1, -1};
        Occupancy occ;
        occ.cov_blocks_per_cu = [&](int, int, bool) { return asked[0] = r[cOccCov]; };
        occ.pow_blocks_per_cu = [&](int, int, int) { return asked[1] = r[cOccPow]; };
        const CovGeom g = choose_cov(c, occ, r[cCovReq]);
        const PowGeom w = choose_pow(c, occ, r[cPowReq]);
        const CovTraits& t = traits(g.kind);
        const int got[kCols - cKind] = {(int)g.kind, g.nsplit, g.tc, g.kc, g.nbg, g.pad, g.part32, partials_f64(g, c.cov_f64) ? 1 : 0, (int)t.unit,
                                        (int)w.kind, w.nb, w.nsplit, w.tcp, w.kp, w.rounds, asked[0], asked[1], c.n_cu};
        bool ok = true;
        for (int i = 0; i < kCols - cKind; ++i) ok = ok && got[i] == r[cKind + i];
        // the traits' own invariants
        const int Mc = c.M + (g.pad && t.padded_x ? 1 : 0);
        ok = ok && t.supported(Mc, c.K) && g.tc % t.quantum == 0 && (long long)g.nsplit * g.tc >= c.T && g.tc % traits(t.unit).quantum == 0;
        ok = ok && traits(t.unit).unit == t.unit && traits(t.unit).partials != Partials::F32IfPart32;
        ok = ok && traits(w.kind).supported(c.M, c.K) && w.tcp % traits(w.kind).quantum == 0 && (long long)w.nsplit * w.tcp >= c.T;
        if (!ok) {
            if (++bad <= 20) {
                std::printf("row %zu differs:", n);
                for (int v : r) std::printf(" %d", v);
                std::printf("\n   chosen here:");
                for (int v : got) std::printf(" %d", v);
                std::printf("\n");
            }
        }
    }
    if (bad) {
        std::printf("%d of %zu rows differ\n", bad, rows.size());
        return 1;
    }
    std::printf("kernel choice ok: %zu rows\n", rows.size());
    return 0;
}
