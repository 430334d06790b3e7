"""Same import path as the reference's src/CGx/utils/membrane_ODE_systems.py."""
from cgx_hip.membrane_odes import (MembraneODESystem, ThreeCompartmentMembraneODESystem,  # noqa: F401
                                   TwoCompartmentMembraneODESystem)
