// GMM background kernels (update and segment): Planar frames of one band, float pixels, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 1, 7, false);
BG_GMM_LAUNCH(float, 1, 8, false);
