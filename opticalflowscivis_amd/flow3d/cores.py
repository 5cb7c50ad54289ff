"""Vortex core lines with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.cores --flows flows.npy --lines-dir
lines --json report.json` finds where the axes of the vortices of every step flow run (parallel vectors: Sujudi-Haimes or
Levy) on the device and links the segments into polylines; see opticalflowscivis_amd/cores.py."""
from ..cores import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model)
