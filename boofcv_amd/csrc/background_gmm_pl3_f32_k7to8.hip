// GMM background kernels (update and segment): Planar frames of three bands, float pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 3, 7, false);
BG_GMM_LAUNCH(float, 3, 8, false);
