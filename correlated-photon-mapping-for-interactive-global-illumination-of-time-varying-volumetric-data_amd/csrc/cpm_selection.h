// cpm_selection.h -- the state of one changed-photon selection, shared by cpm_correlated.hip (select / retrace / finish) and
// cpm_budget.hip (the budgeted finish).
#pragma once
#include "cpm_ctx.h"

// cpm_selection (include/cpm/cpm.h): the state of one changed-photon selection
struct cpm_selection {
    size_t max_photons = 0;
    uint32_t per_tile = 0, max_tiles = 0;
    uint2* tile = nullptr;            // device, max_tiles
    uint32_t* local = nullptr;        // device, max_photons
    int32_t* count_dev = nullptr;     // device
    uint32_t* mask = nullptr;         // device, grow-only: occupancy bits of the importance grid of the last select call
    size_t mask_words = 0;
    const uint32_t* given_mask = nullptr;  // cpm_selection_set_occupancy: the caller's bits (cpm_importance_tf_occupancy) ...
    const float* given_mask_grid = nullptr;  // ... of this importance grid
    unsigned long long* mailbox = nullptr;      // pinned host memory, written by the finish's last launch: [0] = epoch << 32 | listed, [1] = epoch << 32 | changed
    unsigned long long* mailbox_dev = nullptr;  // its device address
    uint32_t n_tiles = 0;             // tiles appended since cpm_selection_begin
    size_t appended_photons = 0;      // ... and the photons they span: no more than that many can be listed
    // cpm_selection_finish_budget: the digit histograms of the rank selection (11 + 10 + 10 key bits) and, per group of
    // kCompactGroup tiles, the listed photons below the cut and on it
    uint32_t* budget_hist = nullptr;  // device, kBudgetHistWords
    uint2* budget_group = nullptr;    // device, ceil(max_tiles / kCompactGroup)
    // cpm_photon_importance_retrace: per launch since cpm_selection_begin (one per light) the order in which its workgroups
    // take the tiles -- costliest first, from the wall-clock the tiles took in the last MEASURED launch (see kRetraceTile)
    struct LaunchOrder { uint32_t n_tiles = 0; uint32_t* order = nullptr; uint32_t* cost = nullptr; uint32_t* keys = nullptr; bool fresh = true; /* no order yet */ };
    std::vector<LaunchOrder> orders;
    std::vector<uint32_t> pending_orders;  // launches measured in this selection: their orders are re-sorted by cpm_selection_finish
    uint32_t n_launches = 0;          // retrace launches since cpm_selection_begin
    uint32_t selections = 0;          // cpm_selection_begin calls
    bool measuring = false;           // this selection's retrace launches record what their tiles cost
    uint32_t epoch = 0;               // of the last cpm_selection_finish enqueued
    bool finished = false;            // a finish has been enqueued since begin
    bool failed = false;              // a select / retrace call since begin failed after its tiles were appended: the finish publishes 0
    hipStream_t last_stream = nullptr;
};

namespace cpm {
constexpr uint32_t kCompactGroup = 16;  // tiles per workgroup of selection_compact_kernel and of the budgeted finish's kernels
constexpr uint32_t kBudgetHistWords = 2048 + 1024 + 1024;
}  // namespace cpm

