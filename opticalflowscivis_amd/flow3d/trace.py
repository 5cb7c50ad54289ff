"""Pathlines with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.trace --dataset droplet3d --size 64
--seed-grid 4 --out traj.npy --json report.json` follows seeded particles through the model's step flows (converted
from the rife3d convention to displacements as evaluate_flow does); see opticalflowscivis_amd/trace.py."""
from ..trace import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
