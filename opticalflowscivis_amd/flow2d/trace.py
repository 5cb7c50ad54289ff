"""Pathlines with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.trace --dataset droplet2d --seed-grid 8
--out traj.npy --json report.json` follows seeded particles through the model's step flows; see
opticalflowscivis_amd/trace.py."""
from ..trace import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
