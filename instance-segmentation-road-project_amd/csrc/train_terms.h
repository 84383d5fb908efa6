// What the trainer's target assignment (train_targets.hip) and its losses (train_losses.hip) share: the launch constants
// and the check of a HIP runtime call.
#pragma once
#include "common.h"

namespace {
namespace tt {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_BLOCKS = ML_TRAIN_MAX_BLOCKS;
constexpr int MAX_CLASSES = ML_EVAL_MAX_CLASSES;
constexpr int MAX_GRID_Y = 65535;

}  // namespace tt
}  // namespace

#define ML_HIP_OK(call, what)                                                \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) {                                              \
            ml_set_error("%s: %s", what, hipGetErrorString(e_));             \
            return ML_E_LAUNCH;                                              \
        }                                                                    \
    } while (0)
