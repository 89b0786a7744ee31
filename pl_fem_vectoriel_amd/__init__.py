"""MI355X-native vectorial H-field P2 FEM eigenmode path (drop-in for the reference ``solver_fem.py``)."""
from .geometry import MCFGeometry, PhotonicLanternGeometry, mcf_positions  # noqa: F401
from .mesh import TriMesh, generate_mesh  # noqa: F401
from .fields import ModeFields, flux_overlap_poses, mode_overlap, mode_overlap_poses, pose_table  # noqa: F401
from .dispersion import mode_dispersion  # noqa: F401
from .nonlinear import mode_nonlinearity  # noqa: F401
from .launch import encircled_na, far_field, field_coupling, gaussian_coupling  # noqa: F401
from .cores import core_decomposition, core_quantities_from_grams  # noqa: F401
from .bend import bend_propagate, bend_quantities_from_grams, bend_response  # noqa: F401
from .profile import IndexProfile, ProfileTangent, ProfiledGeometry  # noqa: F401
from .profile_response import (profile_bend_from_grams, profile_bend_response, profile_dispersion,  # noqa: F401
                               profile_dispersion_from_grams, profile_sensitivity, profile_sensitivity_from_grams)
from .map_gradient import index_map_gradient, index_map_gradient_from_densities  # noqa: F401
from .adapt import adaptive_solve, mark_elements, mode_error_indicators, refine_marked  # noqa: F401
from .splice import (flux_transfer_from_grams, splice_map, splice_power_map, splice_quantities_from_overlaps,  # noqa: F401
                     taper_from_interfaces, taper_transfer, taper_transfer_vectorial)
from .power import Z0_OHM, mode_power, power_quantities_from_grams  # noqa: F401
from .shape import core_velocities, disorder_statistics, shape_response, shape_response_from_grams  # noqa: F401

__all__ = ["MCFGeometry", "PhotonicLanternGeometry", "mcf_positions", "TriMesh", "generate_mesh", "ModeFields", "mode_overlap",
           "mode_dispersion", "mode_nonlinearity", "far_field", "encircled_na", "gaussian_coupling", "field_coupling", "core_decomposition",
           "core_quantities_from_grams", "bend_response", "bend_quantities_from_grams", "bend_propagate", "IndexProfile",
           "ProfiledGeometry", "mode_overlap_poses", "pose_table", "splice_map", "splice_quantities_from_overlaps",
           "taper_from_interfaces", "taper_transfer", "mode_error_indicators", "mark_elements", "refine_marked", "adaptive_solve",
           "mode_power", "power_quantities_from_grams", "Z0_OHM", "flux_overlap_poses", "flux_transfer_from_grams",
           "splice_power_map", "taper_transfer_vectorial", "ProfileTangent", "profile_dispersion", "profile_dispersion_from_grams",
           "profile_sensitivity", "profile_sensitivity_from_grams", "profile_bend_response", "profile_bend_from_grams",
           "core_velocities", "shape_response", "shape_response_from_grams", "disorder_statistics", "index_map_gradient",
           "index_map_gradient_from_densities"]
