// kkt_debug_block_op: one launcher of the time-transform, nullspace and value set-up kernels on
// host data (include/kkt.h documents the arguments).  Nothing here computes: the arrays go up, the
// launcher of kernels.hpp the drivers call runs once on the handle's stream, the arrays come back.
// Arrays the launch writes sit between guards; arrays it only reads are compared with what went up.
#include <algorithm>
#include <cstring>
#include <vector>

#include "system.hpp"

namespace kkt {

namespace {

constexpr size_t G = KKT_BLOCK_GUARD;
constexpr int64_t MAX_ELEMS = (int64_t)1 << 31;   // of one array of a call (16 GiB of doubles)

struct Watch {   // an array the launch must leave as it is
    const void *dev;
    const void *host;
    size_t bytes;
};

struct Arena {
    DevPool pool;
    std::vector<Watch> watched;

    template <class T>
    const T *input(const T *h, size_t n) {
        if (!h) return nullptr;
        const T *d = pool.upload(h, n);
        watched.push_back({d, h, n * sizeof(T)});
        return d;
    }
    // the caller's guarded allocation: guards set here, the array part as it came
    double *output(double *h, size_t n) {
        std::fill(h, h + G, KKT_KRYLOV_PAD);
        std::fill(h + G + n, h + 2 * G + n, KKT_KRYLOV_PAD);
        return pool.upload(h, n + 2 * G) + G;
    }
    uint32_t *flag(uint32_t *h) {
        std::fill(h, h + G, KKT_BLOCK_FLAG_PAD);
        std::fill(h + G + 1, h + 2 * G + 1, KKT_BLOCK_FLAG_PAD);
        return pool.upload(h, 2 * G + 1) + G;
    }
};

[[noreturn]] void bad(const char *what) {
    fail(KKT_ERR_ARG, std::string("kkt_debug_block_op: ") + what);
}

// the n levels' MaskJobs with device pointers; every level without a mask when a.mask is null
const MaskJob *mask_jobs(Arena &A, const kkt_block_op &a, std::vector<MaskJob> &jobs) {
    jobs.assign((size_t)a.n, MaskJob{nullptr, 0.0});
    if (a.mask) {
        const uint8_t *d_mask = A.input(a.mask, (size_t)a.n * a.nx);
        for (int i = 0; i < a.n; ++i) {
            if (a.has_mask && !a.has_mask[i]) continue;
            jobs[i] = MaskJob{d_mask + (size_t)i * a.nx, a.alpha[i]};
        }
    }
    return A.input(jobs.data(), jobs.size());
}

bool any_mask(const kkt_block_op &a) {
    if (!a.mask) return false;
    if (!a.has_mask) return true;
    return std::any_of(a.has_mask, a.has_mask + a.n, [](int32_t v) { return v != 0; });
}

void check_blocks(const kkt_block_op &a) {
    if (a.n < 1 || a.nx < 1) bad("n and nx must be at least 1");
    if (a.nx > MAX_ELEMS / a.n) bad("n * nx is too large");
    if (a.mask && !a.alpha) bad("mask without alpha");
}

void check_indices(const int32_t *idx, int64_t n, int64_t lo, int64_t hi, const char *what) {
    for (int64_t p = 0; p < n; ++p)
        if (idx[p] < lo || idx[p] >= hi) bad(what);
}

void const_jobs(const kkt_block_op &a, std::vector<ConstJob> &jobs, int64_t *max_nx) {
    if (a.n < 1 || a.len < 1 || a.len > MAX_ELEMS) bad("n and len must be at least 1");
    if (!a.job_off || !a.job_nx || !a.job_c1 || !a.job_c2_one || !a.job_c2_alpha)
        bad("null job array");
    jobs.resize((size_t)a.n);
    *max_nx = 0;
    for (int j = 0; j < a.n; ++j) {
        const int64_t off = a.job_off[j], nx = a.job_nx[j];
        if (off < 0 || nx < 1 || off > a.len || nx > a.len - off) bad("a job is not inside [0, len)");
        jobs[j] = ConstJob{off, nx, a.job_c1[j], a.job_c2_one[j], a.job_c2_alpha[j]};
        *max_nx = std::max(*max_nx, nx);
    }
}

}  // namespace

void debug_block_op(System &S, kkt_block_op *pa) {
    if (!pa) bad("null argument");
    kkt_block_op &a = *pa;
    if (a.op < KKT_BLOCK_TIME_TRANSFORM || a.op > KKT_BLOCK_EXTRACT_DINV) bad("unknown op");
    const bool may_alias = a.op == KKT_BLOCK_TIME_TRANSFORM || a.op == KKT_BLOCK_MASK_BLOCKS;
    if (a.in_place && !may_alias) bad("in_place on an operation that has no in-place call");
    if (a.op != KKT_BLOCK_VALS_DIFFER && !a.y) bad("null output array");
    hipStream_t st = S.stream;
    std::vector<MaskJob> mjobs;   // the job lists live until they are compared, below
    std::vector<ConstJob> jobs;
    Arena A;
    // what comes back: (device array part, host allocation, elements of the array part)
    double *d_y = nullptr, *d_y2 = nullptr;
    size_t ny = 0, ny2 = 0;
    uint32_t *d_flag = nullptr;

    switch (a.op) {
        case KKT_BLOCK_TIME_TRANSFORM: {
            if (a.kind < 1 || a.kind > 4) bad("kind must be 1..4");
            check_blocks(a);
            if (!a.in_place && !a.x) bad("null input array");
            ny = (size_t)a.n * a.nx;
            const double *d_x = a.in_place ? nullptr : A.input(a.x, ny);
            const double *d_lo = A.input(a.lo_halo, (size_t)a.nx);
            const double *d_hi = A.input(a.hi_halo, (size_t)a.nx);
            d_y = A.output(a.y, ny);
            launch_time_transform(st, d_y, a.in_place ? d_y : d_x, a.kind, a.n, a.nx, d_lo, d_hi);
            break;
        }
        case KKT_BLOCK_TIME_TRANSFORM_MASK: {
            if (a.kind < 1 || a.kind > 2) bad("kind must be 1 or 2");
            check_blocks(a);
            if (!a.x) bad("null input array");
            if (any_mask(a) && !a.x2) bad("masked levels without xin");
            ny = (size_t)a.n * a.nx;
            const double *d_t = A.input(a.x, ny);
            const double *d_xin = A.input(a.x2, ny);
            const double *d_lo = A.input(a.lo_halo, (size_t)a.nx);
            const double *d_hi = A.input(a.hi_halo, (size_t)a.nx);
            const MaskJob *d_jobs = mask_jobs(A, a, mjobs);
            d_y = A.output(a.y, ny);
            launch_time_transform_mask(st, d_y, d_t, d_xin, d_jobs, a.kind, a.n, a.nx, d_lo, d_hi);
            break;
        }
        case KKT_BLOCK_MASK_BLOCKS: {
            check_blocks(a);
            if (!a.in_place && !a.x) bad("null input array");
            ny = (size_t)a.n * a.nx;
            const double *d_x = a.in_place ? nullptr : A.input(a.x, ny);
            const double *d_mx = A.input(a.x2, ny);
            const MaskJob *d_jobs = mask_jobs(A, a, mjobs);
            d_y = A.output(a.y, ny);
            launch_mask_blocks(st, d_y, a.in_place ? d_y : d_x, d_mx, d_jobs, a.n, a.nx);
            break;
        }
        case KKT_BLOCK_CONST_CORRECT: {
            if (a.kind < 0 || a.kind > 2) bad("second must be 0, 1 or 2");
            int64_t max_nx = 0;
            const_jobs(a, jobs, &max_nx);
            if (!a.y2 || (a.kind && !a.x2)) bad("null array");
            ny = (size_t)a.len;
            ny2 = 2 * (size_t)a.n;
            const double *d_b = a.kind ? A.input(a.x2, ny) : nullptr;
            const ConstJob *d_jobs = A.input(jobs.data(), jobs.size());
            d_y = A.output(a.y, ny);
            d_y2 = A.output(a.y2, ny2);
            launch_const_correct(st, d_jobs, a.n, max_nx, d_y, d_b, a.kind, d_y2);
            break;
        }
        case KKT_BLOCK_CONST_CENTER: {
            int64_t max_nx = 0;
            const_jobs(a, jobs, &max_nx);
            if (!a.x || !a.y2) bad("null array");
            ny = (size_t)a.len;
            ny2 = (size_t)a.n;
            const double *d_x = A.input(a.x, ny);
            const ConstJob *d_jobs = A.input(jobs.data(), jobs.size());
            d_y = A.output(a.y, ny);
            d_y2 = A.output(a.y2, ny2);
            launch_const_center(st, d_jobs, a.n, max_nx, d_x, d_y, d_y2);
            break;
        }
        case KKT_BLOCK_CSR_TO_SELL: {
            if (a.nx < 1 || a.len < 1 || a.nx > MAX_ELEMS || a.len > MAX_ELEMS) bad("bad sizes");
            if (!a.x || !a.idx) bad("null input array");
            check_indices(a.idx, a.nx, -1, a.len, "map entry outside the CSR values");
            ny = (size_t)a.nx;
            const double *d_csr = A.input(a.x, (size_t)a.len);
            const int32_t *d_map = A.input(a.idx, ny);
            d_y = A.output(a.y, ny);
            launch_csr_to_sell(st, d_csr, d_map, d_y, a.nx);
            break;
        }
        case KKT_BLOCK_MASK_COLUMNS: {
            if (a.nx < 1 || a.len < 1 || a.nx > MAX_ELEMS || a.len > MAX_ELEMS) bad("bad sizes");
            if (!a.idx || !a.mask) bad("null input array");
            check_indices(a.idx, a.nx, 0, a.len, "column outside the column mask");
            ny = (size_t)a.nx;
            const int32_t *d_col = A.input(a.idx, ny);
            const uint8_t *d_mask = A.input(a.mask, (size_t)a.len);
            d_y = A.output(a.y, ny);
            launch_mask_columns(st, d_y, d_col, d_mask, a.nx);
            break;
        }
        case KKT_BLOCK_VALS_AXPY: {
            if (a.nx < 1 || a.nx > MAX_ELEMS) bad("bad sizes");
            if (!a.x2) bad("null input array");
            ny = (size_t)a.nx;
            const double *d_a = A.input(a.x, ny);
            const double *d_b = A.input(a.x2, ny);
            d_y = A.output(a.y, ny);
            launch_vals_axpy(st, d_y, d_a, a.c, d_b, a.nx);
            break;
        }
        case KKT_BLOCK_VALS_DIFFER: {
            if (a.nx < 1 || a.nx > MAX_ELEMS) bad("bad sizes");
            if (!a.x || !a.x2 || !a.flag) bad("null array");
            const double *d_a = A.input(a.x, (size_t)a.nx);
            const double *d_b = A.input(a.x2, (size_t)a.nx);
            d_flag = A.flag(a.flag);
            launch_vals_differ(st, d_a, d_b, a.nx, d_flag);
            break;
        }
        case KKT_BLOCK_VALS_SYM_SKEW: {
            if (a.nx < 1 || a.nx > MAX_ELEMS) bad("bad sizes");
            if (!a.x || !a.idx || !a.y2 || !a.flag) bad("null array");
            check_indices(a.idx, a.nx, -1, a.nx, "transposed position outside the values");
            ny = ny2 = (size_t)a.nx;
            const double *d_a = A.input(a.x, ny);
            const int32_t *d_tpos = A.input(a.idx, ny);
            d_y = A.output(a.y, ny);
            d_y2 = A.output(a.y2, ny2);
            d_flag = A.flag(a.flag);
            launch_vals_sym_skew(st, d_a, d_tpos, d_y, d_y2, a.nx, d_flag);
            break;
        }
        case KKT_BLOCK_EXTRACT_DINV: {
            if (a.kind < 1 || a.kind > 2) bad("R must be 1 or 2");
            if (a.n < 1 || a.n > (1 << 20) || a.len < 1 || a.len > MAX_ELEMS) bad("bad sizes");
            if (!a.idx || !a.idx2 || !a.x) bad("null input array");
            const int64_t C = 64 * a.kind, npos = a.n * C;
            if (a.idx2[0] != 0) bad("slice_off must start at 0");
            for (int s = 0; s < a.n; ++s)
                if (a.idx2[s + 1] < a.idx2[s]) bad("slice_off must ascend");
            if (a.nx != (int64_t)a.idx2[a.n] * C) bad("nx must be slice_off[n] * 64 R");
            if (a.idx3)
                check_indices(a.idx3, npos, -1, a.len, "perm entry outside the rows");
            else if (a.len > npos)
                bad("more rows than positions");
            ny = (size_t)a.len;
            const int32_t *d_col = A.input(a.idx, (size_t)a.nx);
            const int32_t *d_off = A.input(a.idx2, (size_t)a.n + 1);
            const double *d_vals = A.input(a.x, (size_t)a.nx);
            const int32_t *d_perm = A.input(a.idx3, (size_t)npos);
            const uint8_t *d_mask = A.input(a.mask, ny);
            d_y = A.output(a.y, ny);
            launch_extract_dinv(st, d_col, d_off, d_vals, d_mask, d_y, (int)a.len, a.n, a.kind,
                                d_perm);
            break;
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    if (d_y)
        HIPCHK(hipMemcpy(a.y, d_y - G, (ny + 2 * G) * sizeof(double), hipMemcpyDeviceToHost));
    if (d_y2)
        HIPCHK(hipMemcpy(a.y2, d_y2 - G, (ny2 + 2 * G) * sizeof(double), hipMemcpyDeviceToHost));
    if (d_flag)
        HIPCHK(hipMemcpy(a.flag, d_flag - G, (2 * G + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int32_t changed = 0;
    std::vector<char> back;
    for (const Watch &w : A.watched) {
        back.resize(w.bytes);
        HIPCHK(hipMemcpy(back.data(), w.dev, w.bytes, hipMemcpyDeviceToHost));
        changed += std::memcmp(back.data(), w.host, w.bytes) != 0;
    }
    a.inputs_changed = changed;
}

}  // namespace kkt
