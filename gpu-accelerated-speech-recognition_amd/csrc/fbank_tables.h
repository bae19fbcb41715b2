// The front end's host-built mel tables and the layout of its device blob and
// of the main kernel's LDS (fbank.hip): what asr_fbank_create
// uploads, reachable without a device.
#pragma once
#include "asr_amd.h"

#include <cstddef>
#include <vector>

namespace asr {

// A work item of the mel stage: bins [s, s + c) of filter f, weights packed[o ..].
struct FbMelItem {
    int s, c, o, f;
};

struct FbTables {
    std::vector<FbMelItem> items;
    std::vector<float> packed;    // each filter's weights from its first to its last non-zero bin
    std::vector<int> idx, filt;   // [n_items][3]: s, c, o;  [n_mels][2]: first item, items
    int n_items, nnz, dct_lds;
    size_t smem;                                              // dynamic LDS bytes of fbank_kernel
    size_t o_tw, o_melw, o_melidx, o_melfilt, o_dct, total;   // blob offsets and size, in floats
};

// mel: the [n_mels][n_fft/2 + 1] matrix of asr_fbank_host_tables; wpb: waves per
// workgroup of the main kernel (2 at n_fft = 2048, else 4).  cfg has passed the
// configuration checks.
void fb_build_tables(const asr_fbank_config* cfg, const float* mel, int wpb, FbTables* t);

}  // namespace asr
