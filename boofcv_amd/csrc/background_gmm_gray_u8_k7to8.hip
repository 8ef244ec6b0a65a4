// GMM background kernels (update and segment): GrayU8 frames, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 1, 7, true);
BG_GMM_LAUNCH(uint8_t, 1, 8, true);
