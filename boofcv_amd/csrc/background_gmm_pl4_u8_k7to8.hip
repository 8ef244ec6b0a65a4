// GMM background kernels (update and segment): Planar frames of four bands, uint8_t pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(uint8_t, 4, 7, false);
BG_GMM_LAUNCH(uint8_t, 4, 8, false);
