"""Same import path as the reference's src/CGx/EMI/EMIx_ionic_model.py."""
from cgx_hip.emi_models import HH_model, IonicModel, Passive_model, g_syn, g_syn_none  # noqa: F401
