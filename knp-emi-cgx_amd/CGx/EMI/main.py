"""Command-line driver with the reference's interface (src/CGx/EMI/main.py):

    python -m CGx.EMI.main --config <file.yaml>

Same construction order: problem -> Hodgkin-Huxley on every membrane tag with the synaptic stimulus -> init_ionic_model ->
SolverEMI(problem, save_xdmfs=True).solve(), then the L2 norms of the two potentials.
"""
from __future__ import annotations

import argparse
from pathlib import Path

from CGx.EMI.EMIx_ionic_model import HH_model, g_syn
from CGx.EMI.EMIx_problem import ProblemEMI
from CGx.EMI.EMIx_solver import SolverEMI


def main_yaml(yaml_file="config.yaml", save_xdmfs=True):
    problem = ProblemEMI(yaml_file)

    HH = HH_model(problem)
    ionic_models = [HH]

    problem.add_ionic_model(ionic_models, problem.gamma_tags, stim_fun=g_syn)
    problem.init_ionic_model(ionic_models)

    solver = SolverEMI(problem, save_xdmfs=save_xdmfs)
    solver.solve()

    phi_i_L2, phi_e_L2 = solver.potential_norms()
    problem.print(f"L2 norm phi_i = {phi_i_L2}")
    problem.print(f"L2 norm phi_e = {phi_e_L2}")
    return solver


def main(argv=None):
    parser = argparse.ArgumentParser(description="EMI on MI355X: the reference's EMI/main.py interface")
    parser.add_argument("--config", dest="config_file", default="./config.yaml", type=Path, help="Configuration file")
    args = parser.parse_args(argv)
    return main_yaml(yaml_file=str(args.config_file))


if __name__ == "__main__":
    main()
