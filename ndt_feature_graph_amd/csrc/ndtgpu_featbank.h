// ndtgpu_featbank.h -- the feature bank's handle, shared by the C-ABI sources that work on its sets: ndtgpu_featmatch.hip (fill,
// match, extract, read back) and ndtgpu_fuser_bank.hip (the fuser's feature term and feature maps).  Host side only and internal,
// like ndtgpu_host.h.
#pragma once
#include "ndtgpu_host.h"
#include "ndt_featmatch.h"

#pragma GCC visibility push(hidden)

struct ndtgpu_featbank {
    NdtFeatBankView v{};                   // what the kernel receives: filled from the owners below at create
    DeviceBuffer<uint32_t> count;
    DeviceBuffer<double> pos, desc;
    // the last host-index match: its indices and outputs
    size_t n_last = 0;
    DeviceBuffer<uint32_t> idx, corr;      // idx: ref indices, then mov indices
    DeviceBuffer<ndtgpu_featmatch_result> results;
    DeviceBuffer<double> T16;
    PinnedBuffer<uint32_t> idx_pin;
    // the last host-range extraction: its inputs and outputs
    size_t n_last_extract = 0;
    DeviceBuffer<uint32_t> ex_idx, ex_beam;
    DeviceBuffer<int32_t> ex_level;
    DeviceBuffer<double> ex_ranges, ex_response;
    DeviceBuffer<ndtgpu_featextract_result> ex_results;
    PinnedBuffer<double> ex_ranges_pin;
    PinnedBuffer<uint32_t> ex_idx_pin;
    Fence used;                            // recorded after the last launch of a call
    Stream hst;                            // set's copies (last: ndtgpu_resource.h)
};

// the device form of a call's RANSAC parameters, checked (ndtgpu_featmatch.hip; prm NULL: the defaults)
ndtgpu_status featmatch_params_dev(const char *what, const ndtgpu_featmatch_params *prm, NdtFeatMatchParamsDev &d);

#pragma GCC visibility pop
