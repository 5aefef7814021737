"""MI355X-native ORB feature front-end (drop-in for the reference's orb.hpp path).

The product is liborbx.so (HIP kernels + C ABI, csrc/); `orbx` is its ctypes view.
The directory name contains a hyphen, so import it with
    importlib.import_module("visual-odometry-gpu_amd")
(see __graft_entry__.load_package()).
"""
from . import (orbx, orbx_carry, orbx_lm, orbx_pnp, orbx_prior, orbx_reloc, orbx_search, orbx_stream, orbx_vo,  # noqa: F401
               shard, streams)
from .orbx import Context, OrbxError, chain_trajectory, default_params  # noqa: F401
