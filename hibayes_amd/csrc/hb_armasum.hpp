// hb_armasum.hpp — arma::sum of a vector as Armadillo's arrayops::accumulate forms it: two interleaved accumulators. Host code.
// The order is the point: sumvx (src/Bayes.cpp:316), yy of the summary-level set-ups and the normalisation of a drawn Pi then
// agree with the reference's to the last bit when their terms do.
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
