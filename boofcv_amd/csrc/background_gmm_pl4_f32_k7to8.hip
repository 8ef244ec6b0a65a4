// GMM background kernels (update and segment): Planar frames of four bands, float pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 4, 7, false);
BG_GMM_LAUNCH(float, 4, 8, false);
