"""Developer tool (GPU box, repo root): ms per step of a manufactured-solution run with the sources and error norms on the host
(``MMS_test: device`` false, the default) and on the device (true), one process, the same mesh:

    python tools/mms_device_measure.py DIM N [STEPS] [host|device|both]

Two warm-up steps (the first one holds the preconditioner set-up and the run-time compilation), then STEPS steps between two device
synchronisations, ``print_errors()`` included as in every MMS run.  Prints one JSON line per path: ms per step, the iterations of the
timed steps, the errors after the last step and, for the device path, the number of registered sources and the launches they add
per step (a volume source: a load launch, a gather and an add per side; a membrane source: one of each)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "knp-emi-cgx_amd")]


def run(dim, N, steps, device):
    import torch
    from parity_utils import mms_config
    from CGx.KNPEMI.KNPEMIx_ionic_model import PassiveModel
    from CGx.KNPEMI.KNPEMIx_problem import ProblemKNPEMI
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = mms_config(dim, N, steps=steps + 2)
    cfg["MMS_test"]["device"] = device
    p = ProblemKNPEMI(cfg)
    p.set_initial_conditions()
    p.init_ionic_models([PassiveModel(p)])
    p.setup_variational_form()
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.prepare()
    for i in (1, 2):
        s.step(i)
    torch.cuda.synchronize()
    tic = time.perf_counter()
    for i in range(3, 3 + steps):
        s.step(i)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - tic) / steps
    srcs = getattr(p, "_sources", None) or []
    out = {"dim": dim, "N": N, "device": bool(device), "steps": steps, "ms_per_step": ms, "iterations": s.iterations[2:], "reasons": s.reasons[2:],
           "n_dof": int(s.backend.n_dof_local), "errors": [float(e) for e in p.errors], "sources": len(srcs),
           "source_launches_per_step": sum(3 * len(h.sides) for h in srcs)}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    dim, N = int(sys.argv[1]), int(sys.argv[2])
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    which = sys.argv[4] if len(sys.argv) > 4 else "both"
    for device in ([False, True] if which == "both" else [which == "device"]):
        run(dim, N, steps, device)
