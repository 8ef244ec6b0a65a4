// GMM background kernels (update and segment): Planar frames of three bands, uint8_t pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 3, 7, false);
BG_GMM_LAUNCH(uint8_t, 3, 8, false);
