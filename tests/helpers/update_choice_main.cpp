// Replays every row of an update-choice table (tools/update_choice_table.py; tests/golden/update_choice.json) through
// choose_update of csrc/kernel_choice.h with the row's switches and compares the normal-form kernel name, and checks the traits'
// own invariants on each row.  Plain C++: no GPU, no HIP.  Prints "update choice ok: N rows, 0 differ" or the rows that differ.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "kernel_choice.h"

using namespace oiva;

namespace {
enum { cM, cK, cDouble, cV64, cInit, cLayout, cNsplit, cGram, cDet, cInverse, cRows, kInts };
struct Row {
    std::vector<int> v;
    std::string kernel;
};

// every integer of text[from, to), in order
std::vector<int> ints(const std::string& s, size_t from, size_t to) {
    std::vector<int> v;
    for (size_t i = from; i < to;) {
        if (s[i] == '-' || (s[i] >= '0' && s[i] <= '9')) {
            size_t used = 0;
            v.push_back(std::stoi(s.substr(i, to - i), &used));
            i += used;
        } else {
            ++i;
        }
    }
    return v;
}

// the packed table (tools/update_choice_table.py): the kernel names once, then per set of switches blocks
// [M, K, layout, nsplit, [k0 .. k7]] whose k at position 4 use_double + 2 vpart_f64 + init_only indexes the names (-1: no row)
std::vector<Row> read_rows(const char* path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string s = ss.str();
    std::vector<Row> rows;
    const size_t k0 = s.find("\"kernels\":["), sets = s.find("\"sets\":[");
    if (k0 == std::string::npos || sets == std::string::npos) return rows;
    std::vector<std::string> kernels;
    for (size_t q = s.find('"', k0 + 10); q != std::string::npos && q < sets; q = s.find('"', q + 1)) {
        const size_t e = s.find('"', q + 1);
        kernels.push_back(s.substr(q + 1, e - q - 1));
        q = e;
    }
    for (size_t at = s.find("\"switches\":[", sets); at != std::string::npos;) {
        const size_t blocks = s.find("\"blocks\":[", at), next = s.find("\"switches\":[", blocks);
        const std::vector<int> sw = ints(s, at, blocks), b = ints(s, blocks, next == std::string::npos ? s.size() : next);
        if (sw.size() != 4 || b.size() % 12 != 0) return {};
        for (size_t i = 0; i < b.size(); i += 12)
            for (int c = 0; c < 8; ++c) {
                const int k = b[i + 4 + c];
                if (k < 0) continue;
                if (k >= (int)kernels.size()) return {};
                rows.push_back({{b[i], b[i + 1], c >> 2, (c >> 1) & 1, c & 1, b[i + 2], b[i + 3], sw[0], sw[1], sw[2], sw[3]}, kernels[k]});
            }
        at = next;
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
        const std::vector<int>& r = rows[n].v;
        if ((int)r.size() != kInts) {
            std::printf("row %zu: %zu integers\n", n, r.size());
            return 2;
        }
        const UpdIn u{r[cM], r[cK], r[cDouble] != 0, r[cV64] != 0, r[cInit] != 0, r[cLayout], r[cNsplit]};
        UpdSwitches sw;
        sw.gram = r[cGram], sw.det = r[cDet] != 0, sw.det16_inverse = r[cInverse] != 0, sw.det16_rows = r[cRows] != 0;
        const UpdChoice c = choose_update(u, sw);
        const std::string got = c.ok ? update_kernel_name(c) : "(none)";
        bool ok = c.ok && got == rows[n].kernel;
        if (c.ok) {
            // the traits' own invariants: the kind takes this channel count and this many splits, the launcher has the
            // instantiation, the workgroup holds whole bins, and the grid covers F bins -- one, a ragged last workgroup, many
            const UpdTraits& t = traits(c.kind);
            ok = ok && u.M >= t.m_lo && u.M <= t.m_hi && (t.max_splits == 0 || u.nsplit <= t.max_splits);
            ok = ok && upd_instantiated(c.kind, c.mp, c.mt, c.kt) && (c.mt == 0 || c.mt == u.M) && (c.kt == 0 || c.kt == u.K);
            ok = ok && c.block == t.block && c.block % 64 == 0 && c.block <= 1024 && c.bins_per_block >= 1;
            if (c.kind <= UpdKind::Det) ok = ok && c.mp >= u.M && c.bins_per_block * c.mp * c.mp == c.block;
            if (c.kind == UpdKind::Rows) ok = ok && c.mp >= u.M && c.bins_per_block * c.mp == c.block;
            for (int F : {1, c.bins_per_block, c.bins_per_block + 1, 2049}) {
                const int grid = ceil_div(F, c.bins_per_block);
                ok = ok && grid >= 1 && grid * c.bins_per_block >= F && (grid - 1) * c.bins_per_block < F;
            }
            // what only one kind may be chosen for
            const bool det_case = u.K == u.M && u.use_double && !u.init_only;
            if (c.kind == UpdKind::Det || c.kind == UpdKind::Det16 || c.kind == UpdKind::Det16Rows) ok = ok && det_case && u.layout == 0;
            if (c.kind == UpdKind::Bg || c.kind == UpdKind::Gram) ok = ok && u.K < u.M && !u.init_only && u.layout == 0;
            if (c.kind == UpdKind::Gram) ok = ok && u.use_double && sw.gram != 0;
            if (c.kind == UpdKind::Wave16) ok = ok && c.flag == (u.K < u.M);
            ok = ok && (c.kind == UpdKind::Rows) == (u.layout != 0 && u.M <= kNarrowMax);
        }
        if (!ok && ++bad <= 20) {
            std::printf("row %zu differs:", n);
            for (int v : r) std::printf(" %d", v);
            std::printf(" recorded %s, chosen here %s\n", rows[n].kernel.c_str(), got.c_str());
        }
    }
    std::printf("update choice %s: %zu rows, %d differ\n", bad ? "DIFFERS" : "ok", rows.size(), bad);
    return bad ? 1 : 0;
}
