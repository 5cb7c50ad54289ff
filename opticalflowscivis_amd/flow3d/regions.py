"""Vortex regions with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.regions --seq frames.npy --criterion both
--out labels.npy --track-ids tracks.npy --json report.json` labels the vortex regions of every step flow (the model's, or
given ones), measures them, links them along the flow and reports tracks and events; see
opticalflowscivis_amd/regions.py."""
from ..regions import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
