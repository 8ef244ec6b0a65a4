// GMM background kernels (update and segment): Planar frames of four bands, uint8_t pixels, 1 to 6 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 4, 1, false);
BG_GMM_LAUNCH(uint8_t, 4, 2, false);
BG_GMM_LAUNCH(uint8_t, 4, 3, false);
BG_GMM_LAUNCH(uint8_t, 4, 4, false);
BG_GMM_LAUNCH(uint8_t, 4, 5, false);
BG_GMM_LAUNCH(uint8_t, 4, 6, false);
