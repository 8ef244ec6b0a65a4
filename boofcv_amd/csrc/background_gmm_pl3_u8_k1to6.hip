// GMM background kernels (update and segment): Planar frames of three bands, uint8_t pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 3, 1, false);
BG_GMM_LAUNCH(uint8_t, 3, 2, false);
BG_GMM_LAUNCH(uint8_t, 3, 3, false);
BG_GMM_LAUNCH(uint8_t, 3, 4, false);
BG_GMM_LAUNCH(uint8_t, 3, 5, false);
BG_GMM_LAUNCH(uint8_t, 3, 6, false);
