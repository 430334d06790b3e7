"""Same import path as the reference's src/CGx/EMI/EMIx_solver.py."""
from cgx_hip.emi_solver import SolverEMI  # noqa: F401
