"""The reference's src/CGx/utils/calc_fluxes.py import path: molar ion fluxes across the membrane, computed on the GPU."""
from cgx_hip.fluxes import compute_fluxes, create_flux_forms  # noqa: F401
