"""The reference's src/CGx/utils/refine_mesh.py command line: ``refine_mesh.py mesh_dir mesh_file facets_file [--levels n]`` writes
``<mesh_file without .xdmf>_refined.xdmf`` with the cell and facet tags carried to the children, refined on the GPU."""
from cgx_hip.refine import main, refine_files  # noqa: F401

if __name__ == "__main__":
    main()
