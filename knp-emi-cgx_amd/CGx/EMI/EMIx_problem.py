"""Same import path as the reference's src/CGx/EMI/EMIx_problem.py."""
from cgx_hip.emi_problem import ProblemEMI  # noqa: F401
