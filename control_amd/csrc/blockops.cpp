// kkt_debug_block_op: one launcher of the time-transform, nullspace and value set-up kernels on
// host data (include/kkt.h documents the arguments).  Nothing here computes: the arrays go up, the
// launcher of kernels.hpp the drivers call runs once on the handle's stream, the arrays come back.
// Arrays the launch writes sit between guards; arrays it only reads are compared with what went up.
// kkt_debug_spectrum_op, below, does the same for the launchers of spectrum_kernels.hip.
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

// ---- kkt_debug_spectrum_op: the same for the launchers of spectrum_kernels.hip.  The scalar state
// of a batch is read and written by one launch, so every guarded array comes back.
namespace {

constexpr bool same(int a, int b) { return a == b; }
static_assert(same(KKT_SPECTRUM_DOT_START, SPEC_DOT_START) && same(KKT_SPECTRUM_DOT_PAP, SPEC_DOT_PAP) &&
              same(KKT_SPECTRUM_DOT_RZ, SPEC_DOT_RZ) && same(KKT_SPECTRUM_DOT_NORM0, SPEC_DOT_NORM0) &&
              same(KKT_SPECTRUM_DOT_NORM, SPEC_DOT_NORM), "kkt.h names the modes of launch_spec_dot");
static_assert(same(KKT_SPECTRUM_UPD_R, SPEC_UPD_R) && same(KKT_SPECTRUM_UPD_P, SPEC_UPD_P) &&
              same(KKT_SPECTRUM_UPD_SCALE, SPEC_UPD_SCALE) && same(KKT_SPECTRUM_UPD_COPY, SPEC_UPD_COPY),
              "kkt.h names the kinds of launch_spec_update");

constexpr int MAX_GRID_Y = 65535;

struct Back {   // a guarded allocation to download
    void *host;
    const void *dev;
    size_t bytes;
};

template <class T>
T pad_of();
template <>
double pad_of<double>() { return KKT_KRYLOV_PAD; }
template <>
uint32_t pad_of<uint32_t>() { return KKT_BLOCK_FLAG_PAD; }
template <>
int32_t pad_of<int32_t>() { return (int32_t)KKT_BLOCK_FLAG_PAD; }
template <>
uint64_t pad_of<uint64_t>() {
    const double d = KKT_KRYLOV_PAD;
    uint64_t u;
    std::memcpy(&u, &d, sizeof u);
    return u;
}

struct SpecArena : Arena {
    std::vector<Back> back;

    template <class T>
    void set_guards(T *h, size_t n) {
        std::fill(h, h + G, pad_of<T>());
        std::fill(h + G + n, h + 2 * G + n, pad_of<T>());
    }
    // the caller's guarded allocation, read and written: comes back whole
    template <class T>
    T *inout(T *h, size_t n) {
        set_guards(h, n);
        T *d = pool.upload(h, n + 2 * G);
        back.push_back({h, d, (n + 2 * G) * sizeof(T)});
        return d + G;
    }
    // a guarded allocation the launch only reads: watched with its guards
    template <class T>
    T *guarded_input(T *h, size_t n) {
        set_guards(h, n);
        return const_cast<T *>(input(h, n + 2 * G)) + G;
    }
};

[[noreturn]] void bad_spec(const char *what) {
    fail(KKT_ERR_ARG, std::string("kkt_debug_spectrum_op: ") + what);
}

void check_batch(const kkt_spectrum_op &a) {
    if (a.nmat < 1 || a.nmat > MAX_GRID_Y || a.n < 1) bad_spec("nmat and n must be at least 1");
    if (a.stride < a.n || (a.stride & 1)) bad_spec("stride must be even and at least n");
    if (a.stride > MAX_ELEMS / a.nmat) bad_spec("nmat * stride is too large");
}

void check_arrays(const kkt_spectrum_op &a) {
    if (a.nmat < 1 || a.nmat > MAX_GRID_Y || a.n < 1) bad_spec("nmat and n must be at least 1");
    if (a.n > MAX_ELEMS / a.nmat) bad_spec("nmat * n is too large");
    if (!a.a) bad_spec("null value arrays");
}

}  // namespace

void debug_spectrum_op(System &S, kkt_spectrum_op *pa) {
    if (!pa) bad_spec("null argument");
    kkt_spectrum_op &a = *pa;
    hipStream_t st = S.stream;
    SpecArena A;
    std::vector<const double *> ptrs;   // the tables live until they are compared, below
    std::vector<SpecSplit> splits;
    std::vector<SpecPair> pairs;
    const unsigned long long *d_words = nullptr;
    int nwords = 0;

    switch (a.op) {
        case KKT_SPECTRUM_DOT: {
            check_batch(a);
            if (a.mode < SPEC_DOT_START || a.mode > SPEC_DOT_NORM) bad_spec("unknown mode");
            if (a.k < 0) bad_spec("k must not be negative");
            if (a.max_steps < 1 || a.max_steps > MAX_ELEMS / a.nmat) bad_spec("bad max_steps");
            if (!a.x || !a.y || !a.active || !a.na || !a.nb || !a.rz || !a.coef || !a.last ||
                !a.mu2 || !a.alpha || !a.beta || !a.part)
                bad_spec("null array");
            for (int b = 0; b < a.nmat; ++b)
                if (a.na[G + b] < 0 || a.nb[G + b] < 0) bad_spec("negative na or nb");
            const size_t nb = (size_t)a.nmat, nvec = nb * (size_t)a.stride;
            const double *d_x = A.input(a.x, nvec);
            const double *d_y = a.y == a.x ? d_x : A.input(a.y, nvec);
            SpecBatch B{};
            B.B = a.nmat;
            B.max_steps = a.max_steps;
            B.n = a.n;
            B.stride = a.stride;
            B.part = A.inout(a.part, nb * REDUCE_BLOCKS);
            B.alpha = A.inout(a.alpha, nb * (size_t)a.max_steps);
            B.beta = A.inout(a.beta, nb * (size_t)a.max_steps);
            B.na = A.inout(a.na, nb);
            B.nb = A.inout(a.nb, nb);
            B.rz = A.inout(a.rz, nb);
            B.coef = A.inout(a.coef, nb);
            B.mu2 = A.inout(a.mu2, nb);
            B.last = A.inout(a.last, nb);
            B.active = A.inout(a.active, nb);
            a.batch_stride = spec_batch_stride(a.n);
            launch_spec_dot(st, B, d_x, d_y, a.mode, a.k);
            break;
        }
        case KKT_SPECTRUM_UPDATE: {
            check_batch(a);
            if (a.mode < SPEC_UPD_R || a.mode > SPEC_UPD_COPY) bad_spec("unknown kind");
            if (!a.x || !a.v || !a.active || !a.coef) bad_spec("null array");
            const size_t nb = (size_t)a.nmat, nvec = nb * (size_t)a.stride;
            double *d_x = const_cast<double *>(A.input(a.x, nvec));
            double *d_v = A.inout(a.v, nvec);
            SpecBatch B{};
            B.B = a.nmat;
            B.max_steps = 1;
            B.n = a.n;
            B.stride = a.stride;
            if (a.mode == SPEC_UPD_R || a.mode == SPEC_UPD_SCALE)
                B.r = d_v;
            else
                B.p = d_v;
            if (a.mode == SPEC_UPD_R)
                B.w = d_x;
            else
                B.z = d_x;
            B.coef = A.guarded_input(a.coef, nb);
            B.active = A.guarded_input(a.active, nb);
            a.batch_stride = spec_batch_stride(a.n);
            launch_spec_update(st, B, a.mode);
            break;
        }
        case KKT_SPECTRUM_SYM_SKEW: {
            check_arrays(a);
            if (!a.tpos || !a.h || !a.sk || !a.flag) bad_spec("null array");
            for (int64_t p = 0; p < a.n; ++p)
                if (a.tpos[p] < -1 || a.tpos[p] >= a.n) bad_spec("transposed position outside the values");
            const size_t nm = (size_t)a.nmat, n = (size_t)a.n;
            const double *d_a = A.input(a.a, nm * n);
            const int32_t *d_tpos = A.input(a.tpos, n);
            double *d_h = A.inout(a.h, nm * n), *d_sk = A.inout(a.sk, nm * n);
            unsigned *d_flag = A.inout(a.flag, nm);
            for (size_t m = 0; m < nm; ++m)
                splits.push_back(SpecSplit{d_a + m * n, d_h + m * n, d_sk + m * n});
            const SpecSplit *d_m = A.input(splits.data(), splits.size());
            launch_spec_sym_skew(st, d_m, a.nmat, d_tpos, a.n, d_flag);
            break;
        }
        case KKT_SPECTRUM_FINGERPRINT: {
            check_arrays(a);
            if (!a.words || !a.fold) bad_spec("null array");
            const size_t nm = (size_t)a.nmat, n = (size_t)a.n;
            nwords = spec_fingerprint_blocks(a.n);
            const double *d_a = A.input(a.a, nm * n);
            for (size_t m = 0; m < nm; ++m) ptrs.push_back(d_a + m * n);
            const double *const *d_vals = A.input(ptrs.data(), ptrs.size());
            static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit words");
            uint64_t *d_w = A.inout(a.words, nm * (size_t)nwords);
            d_words = reinterpret_cast<unsigned long long *>(d_w);
            launch_spec_fingerprint(st, d_vals, a.nmat, a.n, reinterpret_cast<unsigned long long *>(d_w));
            break;
        }
        case KKT_SPECTRUM_PAIRS_DIFFER: {
            check_arrays(a);
            if (a.npairs < 1 || a.npairs > MAX_GRID_Y) bad_spec("npairs must be 1..65535");
            if (!a.pair_a || !a.pair_b || !a.flag) bad_spec("null array");
            for (int q = 0; q < a.npairs; ++q)
                if (a.pair_a[q] < 0 || a.pair_a[q] >= a.nmat || a.pair_b[q] < 0 || a.pair_b[q] >= a.nmat)
                    bad_spec("pair index outside the arrays");
            const size_t nm = (size_t)a.nmat, n = (size_t)a.n;
            const double *d_a = A.input(a.a, nm * n);
            for (int q = 0; q < a.npairs; ++q)
                pairs.push_back(SpecPair{d_a + (size_t)a.pair_a[q] * n, d_a + (size_t)a.pair_b[q] * n});
            const SpecPair *d_pairs = A.input(pairs.data(), pairs.size());
            unsigned *d_flag = A.inout(a.flag, (size_t)a.npairs);
            launch_spec_pairs_differ(st, d_pairs, a.npairs, a.n, d_flag);
            break;
        }
        default: bad_spec("unknown op");
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (const Back &b : A.back) HIPCHK(hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost));
    if (d_words)
        for (int m = 0; m < a.nmat; ++m)
            a.fold[m] = spec_fingerprint_fold(
                reinterpret_cast<const unsigned long long *>(a.words + G + (size_t)m * nwords), nwords);
    int32_t changed = 0;
    std::vector<char> again;
    for (const Watch &w : A.watched) {
        again.resize(w.bytes);
        HIPCHK(hipMemcpy(again.data(), w.dev, w.bytes, hipMemcpyDeviceToHost));
        changed += std::memcmp(again.data(), w.host, w.bytes) != 0;
    }
    a.inputs_changed = changed;
}

}  // namespace kkt
