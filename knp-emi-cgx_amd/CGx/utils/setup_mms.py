"""The reference's src/CGx/utils/setup_mms.py import path: exact solutions and symbolic source terms of the KNP-EMI MMS test."""
from cgx_hip.mms import ExactSolutionsKNPEMI  # noqa: F401
