// Layer shapes the launchers and the weight tables (weight_tables.h) both need: one
// definition each.  Plain C++17, no HIP, so host-only tests can include it.
#pragma once

#include "../../include/mlgate.h"

// LoFTR's ResNetFPN convolutions in mlg_loftr_weights.conv_w order (include/mlgate.h); the
// 196-channel stages padded to 256.  k x k, stride s.
struct ConvSpec {
    int cin, cout, k, s;
};
constexpr ConvSpec CONVS[MLG_LOFTR_NCONV] = {
    {128, 128, 3, 1}, {128, 128, 3, 1}, {128, 128, 3, 1}, {128, 128, 3, 1},                    // layer1
    {128, 256, 3, 2}, {256, 256, 3, 1}, {128, 256, 1, 2}, {256, 256, 3, 1}, {256, 256, 3, 1},  // layer2
    {256, 256, 3, 2}, {256, 256, 3, 1}, {256, 256, 1, 2}, {256, 256, 3, 1}, {256, 256, 3, 1},  // layer3
    {256, 256, 1, 1}, {256, 256, 1, 1}, {256, 256, 3, 1}, {256, 256, 3, 1},                    // FPN 1/4
    {128, 256, 1, 1}, {256, 256, 3, 1}, {256, 128, 3, 1}};                                     // FPN 1/2

// torchvision ResNet-50's bottleneck stages: width and block count (a block's output has
// 4 * width channels; the first block of a stage carries the downsample conv)
constexpr int RN_STAGES = 4;
constexpr int RN_WIDTHS[RN_STAGES] = {64, 128, 256, 512}, RN_NBLOCKS[RN_STAGES] = {3, 4, 6, 3};

// SuperPoint's bf16 layers in mlg_sp_weights.w order: conv1b conv2a conv2b conv3a conv3b
// conv4a conv4b convPa convPb convDa convDb.  cout: rows stored (convPb: 65 padded to 128)
struct SpLayer {
    int cin, cout, k;
};
constexpr SpLayer SP_LAYERS[11] = {{64, 64, 3},   {64, 64, 3},   {64, 64, 3},   {64, 128, 3},
                                   {128, 128, 3}, {128, 128, 3}, {128, 128, 3}, {128, 256, 3},
                                   {256, 128, 1}, {128, 256, 3}, {256, 256, 1}};
