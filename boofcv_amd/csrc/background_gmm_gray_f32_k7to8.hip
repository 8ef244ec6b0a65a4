// GMM background kernels (update and segment): GrayF32 frames, 7 to 8 Gaussians.
#include "background_dev.h"

BG_GMM_LAUNCH(float, 1, 7, true);
BG_GMM_LAUNCH(float, 1, 8, true);
