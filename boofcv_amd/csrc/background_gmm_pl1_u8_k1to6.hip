// GMM background kernels (update and segment): Planar frames of one band, uint8_t pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 1, 1, false);
BG_GMM_LAUNCH(uint8_t, 1, 2, false);
BG_GMM_LAUNCH(uint8_t, 1, 3, false);
BG_GMM_LAUNCH(uint8_t, 1, 4, false);
BG_GMM_LAUNCH(uint8_t, 1, 5, false);
BG_GMM_LAUNCH(uint8_t, 1, 6, false);
