// snpmodel_sanitize.cpp -- the checks and logs of the SNP-call matrices (csrc/npr_snpmodel.h) under AddressSanitizer and UBSan: every matrix
// is a heap block of exactly its size, so a read or write past n_models matrices is a heap-buffer-overflow report, and a refused call must
// leave its outputs as they were.  A host program, built and run on the CPU by `make -C nanopore_amd/csrc check-snpmodel`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "npr_snpmodel.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

// a heap copy of exactly n doubles
double *block(const std::vector<double> &v) {
    double *p = static_cast<double *>(std::malloc(v.size() * sizeof(double) + (v.empty() ? 1 : 0)));
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

std::vector<double> flat_error(int n_models) {
    std::vector<double> e;
    for (int m = 0; m < n_models; ++m)
        for (int i = 0; i < 16; ++i) e.push_back(i / 4 == i % 4 ? 0.8 - 0.01 * m : (0.2 + 0.01 * m) / 3);
    return e;
}

// one call on exact-size blocks: -> accepted; the outputs are untouched when it is not
bool call(int n_models, const std::vector<double> &evolution, const std::vector<double> &error, std::vector<double> *logs = nullptr) {
    const int held = n_models >= 1 && n_models <= npr::kSnpMaxModels ? n_models : 0;
    double *ev = block(evolution), *er = block(error);
    const double mark = -12345.0;
    double *le = block(std::vector<double>(16, mark)), *lr = block(std::vector<double>(16 * static_cast<size_t>(held), mark));
    const bool ok = npr::snp_log_matrices(n_models, ev, er, le, lr);
    if (!ok) {
        for (int i = 0; i < 16; ++i) EXPECT(le[i] == mark);
        for (int i = 0; i < 16 * held; ++i) EXPECT(lr[i] == mark);
    } else {
        for (int i = 0; i < 16; ++i) EXPECT(le[i] == std::log(evolution[i]));
        for (int i = 0; i < 16 * held; ++i) EXPECT(lr[i] == std::log(error[i]) && std::isfinite(lr[i]));
        if (logs) logs->assign(le, le + 16);
    }
    std::free(ev), std::free(er), std::free(le), std::free(lr);
    return ok;
}

}  // namespace

int main() {
    const std::vector<double> ones(16, 1.0);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int n = 1; n <= npr::kSnpMaxModels; ++n) EXPECT(call(n, ones, flat_error(n)));
    EXPECT(!call(0, ones, flat_error(1)));
    EXPECT(!call(npr::kSnpMaxModels + 1, ones, flat_error(npr::kSnpMaxModels + 1)));
    EXPECT(!call(-1, ones, flat_error(1)));
    EXPECT(!npr::snp_log_matrices(1, nullptr, nullptr, nullptr, nullptr));
    // every error entry of every model is looked at, and no entry beyond them
    for (int n = 1; n <= npr::kSnpMaxModels; ++n)
        for (int i = 0; i < 16 * n; ++i)
            for (double bad : {0.0, -0.25, nan, inf, -inf}) {
                std::vector<double> e = flat_error(n);
                e[static_cast<size_t>(i)] = bad;
                EXPECT(!call(n, ones, e));
            }
    EXPECT(call(1, ones, std::vector<double>(16, std::numeric_limits<double>::denorm_min())));  // the smallest number above zero: a finite log
    // a zero evolution entry is allowed (-inf) while its row keeps a possible candidate
    std::vector<double> ev = ones, logs;
    ev[1] = ev[6] = 0.0;
    EXPECT(call(2, ev, flat_error(2), &logs));
    EXPECT(logs.size() == 16 && logs[1] == -inf && logs[6] == -inf && logs[0] == 0.0);
    for (int r = 0; r < 4; ++r) {
        std::vector<double> z = ones;
        for (int c = 0; c < 4; ++c) z[static_cast<size_t>(4 * r + c)] = 0.0;
        EXPECT(!call(1, z, flat_error(1)));
    }
    for (int i = 0; i < 16; ++i)
        for (double bad : {-1.0, nan, inf}) {
            std::vector<double> z = ones;
            z[static_cast<size_t>(i)] = bad;
            EXPECT(!call(1, z, flat_error(1)));
        }
    if (failures) {
        std::printf("snpmodel_sanitize: %d failures\n", failures);
        return 1;
    }
    std::printf("snpmodel_sanitize ok\n");
    return 0;
}
