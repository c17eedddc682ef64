// hb_armasum.hpp — arma::sum of a vector as Armadillo's accumulate forms it: two interleaved accumulators. Host code; shared by the
// summary-level units (hb_sbayes.hip, hb_cg.hip), whose set-ups must sum yyi exactly as the reference does.
#pragma once
#include <stddef.h>

static inline double arma_sum(const double *v, size_t n)
{
    double a1 = 0.0, a2 = 0.0;
    size_t j;
    for (j = 1; j < n; j += 2) {
        a1 += v[j - 1];
        a2 += v[j];
    }
    if ((j - 1) < n) a1 += v[j - 1];
    return a1 + a2;
}
