// mixture_set.hpp -- the in-memory mixture set behind amx_mixture_set (include/amx.h): what amx_pms_read, amx_gmm_estimate and
// amx_ebw_estimate hand out and amx_mixture_set_view shows.  Shared by pms_io.cpp and ebw_host.cpp.
#pragma once
#include <cstdint>
#include <vector>

struct amx_mixture_set {
    int                   dim = 0;
    std::vector<uint32_t> mix_off, dens_index, dens_mean, dens_cov;
    std::vector<double>   log_weight;
    std::vector<float>    means, variances;
};
