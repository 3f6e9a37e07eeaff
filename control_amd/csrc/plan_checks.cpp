// The host-only checks of compose.hpp: nothing of HIP beyond fail().
#include "compose.hpp"
#include "system.hpp"

namespace kkt {

static void need(bool ok, const std::string &what, const char *msg) {
    if (!ok) fail(KKT_ERR_ARG, what + ": " + msg);
}

void check_csr(const std::string &what, const int32_t *ip, const int32_t *ix, int64_t nrows,
               int64_t ncols, int64_t nnz) {
    need(ip && ix, what, "null pattern");
    need(ip[0] == 0 && ip[nrows] == nnz, what, "indptr does not span nnz");
    for (int64_t r = 0; r < nrows; ++r) {
        // (a row's end within nnz before its entries are read: ip[nrows] == nnz alone does not
        // bound a row that overshoots and comes back)
        need(ip[r] <= ip[r + 1] && ip[r + 1] <= nnz, what, "indptr decreases");
        for (int32_t k = ip[r]; k < ip[r + 1]; ++k) {
            need(ix[k] >= 0 && ix[k] < ncols, what, "column out of range");
            need(k == ip[r] || ix[k - 1] < ix[k], what, "columns not sorted");
        }
    }
}

void check_lists(const std::string &what, const int32_t *cptr, const int32_t *clist, int64_t nnz,
                 int64_t n_entries) {
    need(cptr && clist, what, "null contribution list");
    need(cptr[0] == 0 && cptr[nnz] == n_entries, what,
         "the lists must hold every element entry once");
    for (int64_t k = 0; k < nnz; ++k) {
        need(cptr[k] <= cptr[k + 1] && cptr[k + 1] <= n_entries, what, "list pointer decreases");
        for (int32_t j = cptr[k]; j < cptr[k + 1]; ++j)
            need(clist[j] >= 0 && clist[j] < n_entries &&
                     (j == cptr[k] || clist[j - 1] < clist[j]),
                 what, "list entries out of range or not ascending");
    }
}

void check_perm(const std::string &what, const int32_t *t, int64_t nnz) {
    need(t != nullptr, what, "null transpose permutation");
    for (int64_t k = 0; k < nnz; ++k)
        need(t[k] >= 0 && t[k] < nnz && t[t[k]] == k, what, "not a transpose permutation");
}

void check_range(const std::string &what, const int32_t *idx, int64_t n, int64_t bound) {
    for (int64_t k = 0; k < n; ++k) need(idx[k] >= 0 && idx[k] < bound, what, "index out of range");
}

bool pattern_is_space(const Pattern &Q, const ComposeSpace &sp) {
    const int64_t n = (int64_t)sp.indptr.size() - 1, nnz = sp.nnz, c = sp.ncomp;
    if (n <= 0 || Q.nrows != c * n || Q.ncols != c * n || Q.nnz != c * nnz) return false;
    if ((int64_t)Q.h_indptr.size() != c * n + 1 || (int64_t)Q.h_indices.size() != c * nnz)
        return false;
    for (int64_t row = 0; row <= c * n; ++row) {
        const int64_t comp = row == c * n ? c - 1 : row / n;
        if (Q.h_indptr[row] != comp * nnz + sp.indptr[row - comp * n]) return false;
    }
    for (int64_t k = 0; k < c * nnz; ++k)
        if (Q.h_indices[k] != (k / nnz) * n + sp.indices[k % nnz]) return false;
    return true;
}

}  // namespace kkt
