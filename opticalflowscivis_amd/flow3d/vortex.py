"""Vortex and divergence fields with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.vortex --seq frames.npy
--fields div,vmag,q,l2 --out vg.npy --mask m.npy --json report.json` differentiates the model's step flows into
divergence, vorticity, Q and lambda2 on the device; see opticalflowscivis_amd/vortex.py."""
from ..vortex import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
