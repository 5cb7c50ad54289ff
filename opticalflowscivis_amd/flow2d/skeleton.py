"""Topological skeletons with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.skeleton --dataset rectangle2d
--png-dir shots --json report.json` finds the saddles of the step flows, traces the four separatrices of each on the
device, reports which sink, source or saddle each ends in and draws them over the frames; see
opticalflowscivis_amd/skeleton.py."""
from ..skeleton import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
