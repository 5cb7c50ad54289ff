"""Critical points with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.critical --dataset rectangle2d
--png-dir shots --json report.json` finds where the step flows vanish and names each zero (sink, saddle, source, focus)
on the device, links the zeros of consecutive steps and draws them over the frames; see opticalflowscivis_amd/critical.py."""
from ..critical import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
