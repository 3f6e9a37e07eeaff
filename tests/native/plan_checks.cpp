// The host-side checks of the re-linearisation plans (control_amd/csrc/plan_checks.cpp) on the P1
// pattern of a 3 x 3-node mesh: every validator accepts the correct arrays and refuses one fault
// each with KKT_ERR_ARG and the caller's prefix, and pattern_is_space tells a correct one- and
// two-component target from wrong ones.  A program of its own (tests/test_plan_checks.py builds
// it plain and under the address and undefined-behaviour sanitizers): no GPU, no HIP call.
#include <algorithm>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "../../control_amd/csrc/compose.hpp"
#include "../../control_amd/csrc/system.hpp"

namespace kkt {
void fail(int code, const std::string &m) { throw Error{code, m}; }
}  // namespace kkt

using namespace kkt;
using I32 = std::vector<int32_t>;

static int failures = 0;
static const std::string PREFIX = "kkt_test_entry: the array";

static void accepted(const char *name, const std::function<void()> &f) {
    try {
        f();
    } catch (const Error &e) {
        std::printf("FAILED %s: refused (%d) %s\n", name, e.code, e.msg.c_str());
        ++failures;
    }
}

static void refused(const char *name, const std::function<void()> &f) {
    try {
        f();
    } catch (const Error &e) {
        if (e.code != KKT_ERR_ARG || e.msg.compare(0, PREFIX.size() + 2, PREFIX + ": ") != 0) {
            std::printf("FAILED %s: code %d, message '%s'\n", name, e.code, e.msg.c_str());
            ++failures;
        }
        return;
    }
    std::printf("FAILED %s: accepted\n", name);
    ++failures;
}

static void expect(const char *name, bool got, bool want) {
    if (got != want) {
        std::printf("FAILED %s: %d, expected %d\n", name, (int)got, (int)want);
        ++failures;
    }
}

// ncomp copies of the scalar pattern, component-major
static Pattern target(const I32 &ip, const I32 &ix, int ncomp) {
    const int32_t n = (int32_t)ip.size() - 1, nnz = (int32_t)ix.size();
    Pattern Q;
    Q.nrows = Q.ncols = (int64_t)ncomp * n;
    Q.nnz = (int64_t)ncomp * nnz;
    Q.h_indptr.push_back(0);
    for (int c = 0; c < ncomp; ++c) {
        for (int32_t r = 1; r <= n; ++r) Q.h_indptr.push_back(c * nnz + ip[r]);
        for (int32_t k = 0; k < nnz; ++k) Q.h_indices.push_back(c * n + ix[k]);
    }
    return Q;
}

int main() {
    // 3 x 3 nodes, 2 x 2 squares of two triangles each
    const int32_t nn = 9;
    std::vector<std::vector<int32_t>> cells;
    for (int32_t j = 0; j < 2; ++j)
        for (int32_t i = 0; i < 2; ++i) {
            const int32_t a = 3 * j + i, b = a + 1, c = a + 3, d = a + 4;
            cells.push_back({a, b, d});
            cells.push_back({a, d, c});
        }
    std::vector<std::vector<int32_t>> rows(nn);
    for (auto &t : cells)
        for (int32_t r : t)
            for (int32_t c : t) rows[r].push_back(c);
    I32 ip{0}, ix;
    for (auto &r : rows) {
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        ix.insert(ix.end(), r.begin(), r.end());
        ip.push_back((int32_t)ix.size());
    }
    const int32_t nnz = (int32_t)ix.size();
    auto position = [&](int32_t r, int32_t c) {
        return (int32_t)(std::lower_bound(ix.begin() + ip[r], ix.begin() + ip[r + 1], c) -
                         ix.begin());
    };
    I32 tperm(nnz);
    for (int32_t r = 0; r < nn; ++r)
        for (int32_t k = ip[r]; k < ip[r + 1]; ++k) tperm[k] = position(ix[k], r);
    // contribution lists: entry 9 e + 3 a + b adds to the position of (cell[a], cell[b])
    const int32_t n_entries = 9 * (int32_t)cells.size();
    std::vector<I32> at(nnz);
    for (int32_t e = 0; e < (int32_t)cells.size(); ++e)
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b)
                at[position(cells[e][a], cells[e][b])].push_back(9 * e + 3 * a + b);
    I32 cptr{0}, clist;
    for (auto &l : at) {
        clist.insert(clist.end(), l.begin(), l.end());
        cptr.push_back((int32_t)clist.size());
    }

    // ---- validators
    accepted("csr", [&] { check_csr(PREFIX, ip.data(), ix.data(), nn, nn, nnz); });
    accepted("perm", [&] { check_perm(PREFIX, tperm.data(), nnz); });
    accepted("lists", [&] { check_lists(PREFIX, cptr.data(), clist.data(), nnz, n_entries); });
    accepted("range", [&] { check_range(PREFIX, ix.data(), nnz, nn); });
    {
        I32 bad = ip;
        bad[nn] = nnz - 1;
        refused("indptr not spanning nnz",
                [&] { check_csr(PREFIX, bad.data(), ix.data(), nn, nn, nnz); });
        bad = ip;
        bad[4] = bad[3] - 1;
        refused("decreasing indptr", [&] { check_csr(PREFIX, bad.data(), ix.data(), nn, nn, nnz); });
        bad = ip;
        bad[4] = nnz + 100;   // ... and one that first runs past the arrays
        refused("overshooting indptr",
                [&] { check_csr(PREFIX, bad.data(), ix.data(), nn, nn, nnz); });
    }
    {
        I32 bad = ix;
        bad[nnz - 1] = nn;
        refused("column out of range", [&] { check_csr(PREFIX, ip.data(), bad.data(), nn, nn, nnz); });
        bad = ix;
        bad[0] = -1;
        refused("negative column", [&] { check_csr(PREFIX, ip.data(), bad.data(), nn, nn, nnz); });
        bad = ix;
        std::swap(bad[ip[4]], bad[ip[4] + 1]);
        refused("unsorted columns", [&] { check_csr(PREFIX, ip.data(), bad.data(), nn, nn, nnz); });
        refused("index out of range", [&] { check_range(PREFIX, ix.data(), nnz, nn - 1); });
    }
    {
        I32 bad = tperm;   // a permutation still, but of order three on the positions 1, 2, 3
        bad[1] = 2, bad[2] = 3, bad[3] = 1;
        refused("non-involutive tperm", [&] { check_perm(PREFIX, bad.data(), nnz); });
        bad = tperm;
        bad[0] = nnz;
        refused("tperm out of range", [&] { check_perm(PREFIX, bad.data(), nnz); });
    }
    {
        I32 short_list(clist.begin(), clist.end() - 1), bad = cptr;
        bad[nnz] = n_entries - 1;
        refused("a list that misses an entry",
                [&] { check_lists(PREFIX, bad.data(), short_list.data(), nnz, n_entries); });
        int32_t k = 0;
        while (cptr[k + 1] - cptr[k] < 2) ++k;
        I32 desc = clist;
        std::swap(desc[cptr[k]], desc[cptr[k] + 1]);
        refused("a descending list",
                [&] { check_lists(PREFIX, cptr.data(), desc.data(), nnz, n_entries); });
        bad = cptr;
        bad[2] = n_entries + 100;
        refused("an overshooting list pointer",
                [&] { check_lists(PREFIX, bad.data(), clist.data(), nnz, n_entries); });
    }

    // ---- the proof that a target pattern is a space's
    ComposeSpace one, two;
    one.indptr = two.indptr = ip;
    one.indices = two.indices = ix;
    one.nnz = two.nnz = nnz;
    two.ncomp = 2;
    const Pattern Q1 = target(ip, ix, 1), Q2 = target(ip, ix, 2);
    expect("one component", pattern_is_space(Q1, one), true);
    expect("two components", pattern_is_space(Q2, two), true);
    expect("one component asked of a two-component target", pattern_is_space(Q2, one), false);
    expect("two components asked of a one-component target", pattern_is_space(Q1, two), false);
    {
        Pattern Q = Q2;   // the second component's columns one to the left
        for (int32_t k = nnz; k < 2 * nnz; ++k) Q.h_indices[k] -= 1;
        expect("second half: columns shifted by one", pattern_is_space(Q, two), false);
        Q = Q2;           // ... its rows one position late
        for (int32_t r = nn + 1; r < 2 * nn; ++r) Q.h_indptr[r] += 1;
        expect("second half: row ends shifted by one", pattern_is_space(Q, two), false);
        Q = Q1;
        Q.h_indices[nnz - 1] -= 1;
        expect("one column changed", pattern_is_space(Q, one), false);
        Q = Q1;
        Q.h_indptr.pop_back();   // sizes that contradict the header: nothing is read past them
        expect("a short indptr", pattern_is_space(Q, one), false);
    }
    std::printf("plan checks: %d failures\n", failures);
    return failures ? 1 : 0;
}
