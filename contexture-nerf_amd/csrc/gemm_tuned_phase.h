// Tuned plans of the upsampling convolutions in their phase form (GemmArgs::phase; tools/tune_gemm.py --phase 1 on MI355X), in a table
// of their own: gemm_tuned.h keeps the nine-tap rows of the same layers, which an engine without a derived blob still runs.
// Rows as in gemm_tuned.h; flags = 6 (bit 1 fused x2 upsample, bit 2 its phase form), K = 4 Cin, M = the output's pixels.
// The UNet's three upsamplers at latent 96^2 (CFG batch 2 and the lockstep batch 12) and on the Zero123++ grid (latent 120 x 80), and
// the VAE decoder's three at 768^2.
#pragma once
static const TunedGemm g_tuned_phase[] = {
    {1, 1152, 1280, 5120, 6, 0, -1, 7, 4},   // 29.9 us (was 32.9)
    {1, 4608, 1280, 5120, 6, 0, -1, 6, 1},   // 66.6 us (was 66.1)
    {1, 18432, 640, 2560, 6, 0, -1, 8, 1},   // 68.8 us (was 86.1)
    {1, 1200, 1280, 5120, 6, 0, 25, 0, 2},   // 32.8 us (was 32.8)
    {1, 4800, 1280, 5120, 6, 0, 10, 0, 1},   // 80.7 us (was 112.4)
    {1, 19200, 640, 2560, 6, 0, 20, 0, 1},   // 84.3 us (was 111.2)
    {1, 36864, 512, 2048, 6, 0, 20, 0, 1},   // 99.8 us (was 119.5)
    {1, 147456, 512, 2048, 6, 0, 20, 0, 1},   // 358.9 us (was 376.8)
    {1, 589824, 256, 1024, 6, 0, 20, 0, 1},   // 406.8 us (was 456.8)
    {1, 6912, 1280, 5120, 6, 0, -1, 8, 1},   // 104.6 us (was 114.8)
    {1, 27648, 1280, 5120, 6, 0, -1, 8, 1},   // 358.7 us (was 355.2)
    {1, 110592, 640, 2560, 6, 0, -1, 8, 1},   // 377.8 us (was 382.1)
};
