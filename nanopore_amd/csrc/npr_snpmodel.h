// npr_snpmodel.h -- the substitution matrices of the SNP calls (include/nprealign.h: npr_*_snp_calls) from the caller's probabilities to
// what k_snp_calls (npr_snpcall.hip) takes: checked, then natural logs in fp64.  Standard library only, so that a host program without HIP
// can run it under a sanitizer (tests/native/snpmodel_sanitize.cpp).  Not installed.
#pragma once
#include <cmath>
#include <cstdint>

namespace npr {

constexpr int kSnpMaxModels = 4;  // NPR_SNP_MAX_MODELS (npr_snp_api.cpp asserts that they agree)

// log_evolution[16] = log evolution16 ([reference][candidate]; a zero gives -inf: that candidate gets p = 0),
// log_error[n_models][16] = log error16 ([candidate][observed]).  false, with nothing written: n_models outside 1..kSnpMaxModels, a null
// matrix, an evolution entry that is negative or not finite, a reference base none of whose candidates is possible, or an error entry
// that is not a finite number above zero (the host path's 0 * log 0 is a NaN).
inline bool snp_log_matrices(int32_t n_models, const double *evolution16, const double *error16, double *log_evolution, double *log_error) {
    if (n_models < 1 || n_models > kSnpMaxModels || !evolution16 || !error16) return false;
    for (int r = 0; r < 4; ++r) {
        bool any = false;
        for (int c = 0; c < 4; ++c) {
            const double v = evolution16[4 * r + c];
            if (!(v >= 0.0) || !std::isfinite(v)) return false;
            any = any || v > 0.0;
        }
        if (!any) return false;
    }
    for (int i = 0; i < 16 * n_models; ++i)
        if (!(error16[i] > 0.0) || !std::isfinite(error16[i])) return false;
    for (int i = 0; i < 16; ++i) log_evolution[i] = std::log(evolution16[i]);  // (log 0 = -inf)
    for (int i = 0; i < 16 * n_models; ++i) log_error[i] = std::log(error16[i]);
    return true;
}

}  // namespace npr
