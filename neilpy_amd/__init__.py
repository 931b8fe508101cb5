"""neilpy_amd: MI355X-native implementation of neilpy's SMRF bare-earth path.

Drop-in for ``neilpy.smrf`` / ``progressive_filter`` / ``create_dem`` /
``inpaint_nans_by_springs`` (and the ``disk`` / ``opening`` seam they use).  All compute runs
in hand-written gfx950 HIP kernels in ``libsmrf_hip.so`` (C ABI: ``include/smrf_hip.h``);
there is no CPU fallback.  ``openness`` / ``skyview_factor`` / ``geomorphons`` and their kin (neilpy_amd/terrain.py)
analyse the resulting DTM with the same kernels-only rule, and so do its local surface derivatives ``slope`` / ``aspect``
/ ``hillshade`` / the curvatures (neilpy_amd/surface.py).  ``inpaint_nearest`` is the third hole filler, an exact nearest-cell
infill, and ``nearest_source`` the distance / index planes behind it (neilpy_amd/nearest.py).  ``focal_convolve`` is
``scipy.ndimage.convolve(mode='nearest')`` bit for bit, and ``std`` / ``topographic_position_index`` / ``reduce_peaks``
rest on it (neilpy_amd/focal.py).  ``scaled_morphometry`` / ``vip_score`` / ``ashift`` are the multi-scale tools, strided
stencils under ashift's edge rule, with the host helper ``triangle_height`` (neilpy_amd/morphometry.py).
``chamfer_distance`` compares two point clouds and ``nearest_points`` is the exact nearest-neighbour query under it, a
counting sort into a cell grid and a ring search (neilpy_amd/points.py).  ``voxelize`` turns a cloud into the boolean
voxel model ``np.histogramdd`` and a threshold give, bit for bit: a scatter into a bit set and a byte expansion with the
bottom fill (neilpy_amd/voxel.py).  ``colortable_shade`` / ``swiss_shading`` / ``brassel_atmospheric_perspective`` turn a DTM and its
hillshade into the coloured relief image, over ``raster_stats`` (NaN-ignoring moments in a fixed summation order and an
exact radix-select median), ``normalize`` and ``rmse`` (neilpy_amd/relief.py).  ``hungarian_algorithm`` matches two
point sets at the least total distance, ``bdr`` is the bidimensional regression and ``bdr_bootstrap`` its bootstrap over
matched samples: one wave64 per assignment problem, shortest augmenting paths out of LDS, every sample of the bootstrap
solved and regressed in one launch (neilpy_amd/matching.py).  ``grey_erosion`` / ``grey_dilation`` / ``grey_opening`` /
``grey_closing`` / ``white_tophat`` / ``black_tophat`` / ``morphological_gradient`` are ``scipy.ndimage``'s grey
morphology for any flat footprint (``size=`` or ``footprint=``, modes 'reflect' and 'nearest') bit for bit, with the host
helpers ``rectangle`` / ``square`` / ``diamond``: a tap kernel and an LDS kernel that takes each run of consecutive
members from two reads of a power-of-two min / max plane (neilpy_amd/morphology.py).
"""
from ._lib import SmrfHipError, load as load_library, LIB_PATH          # noqa: F401
from .affine import Affine, edges_from_IT, from_origin, write_worldfile                 # noqa: F401
from .api import (create_dem, dilation, disk, erosion, inpaint_nans_by_fda, inpaint_nans_by_springs,   # noqa: F401
                  last_stats,
                  opening, progressive_filter, pssm, smrf)
from .focal import distance_kernel, focal_convolve, reduce_peaks, std, topographic_position_index   # noqa: F401
from .las import read_las, read_las_xyz, write_las                         # noqa: F401
from .matching import bdr, bdr_bootstrap, hungarian_algorithm              # noqa: F401
from .morphology import (black_tophat, diamond, grey_closing, grey_dilation, grey_erosion, grey_opening,   # noqa: F401
                         morphological_gradient, rectangle, square, white_tophat)
from .morphometry import ashift, scaled_morphometry, triangle_height, vip_score   # noqa: F401
from .nearest import inpaint_nearest, nearest_source                      # noqa: F401
from .points import chamfer_distance, nearest_points                       # noqa: F401
from .relief import (brassel_atmospheric_perspective, colortable_shade, cutter, normalize, raster_stats,   # noqa: F401
                     rmse, swiss_shading)
from .surface import (aspect, curvature, esri_curvature, esri_slope, evans_curvature, hillshade,   # noqa: F401
                      multiple_illumination, slope, wilson_gallant_curvature, z_factor,
                      zevenbergen_and_thorne_curvature)
from .synth import synth_dem, synth_points                               # noqa: F401
from .voxel import voxelize                                                # noqa: F401
from .terrain import (count_openness, geomorphon_cmap, geomorphons, get_lowest_equivalent, int2base,   # noqa: F401
                      openness, progressive_window, skyview_factor, ternary_pattern_from_openness,
                      terrain_code_to_geomorphon)

__version__ = "0.1.0"
