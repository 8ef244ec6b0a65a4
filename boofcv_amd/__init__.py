"""boofcv_amd -- MI355X (gfx950) provider for BoofCV's detect -> describe -> associate hot path.

The product is boofcv_amd/libboofhip.so (hand-written HIP kernels behind the C ABI of include/boofhip.h);
the `boofcv_amd.api` package mirrors the reference's Java interfaces on top of it, one module per family.  Nothing here falls back to the CPU.
"""
from . import _lib  # noqa: F401
from .api import *  # noqa: F401,F403
from .binary import *  # noqa: F401,F403  (thresholding: a module beside the api package)
from .census import *  # noqa: F401,F403  (census transform and census block matching: likewise)
from .best5 import *  # noqa: F401,F403  (five-region block matching, blockMatchBest5: likewise)

__version__ = "0.1"
