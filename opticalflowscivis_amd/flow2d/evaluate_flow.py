"""Flow evaluation with the Flow-2D model: `python -m opticalflowscivis_amd.flow2d.evaluate_flow --dataset droplet2d
--gap 2 --zero-baseline --out result.json` scores the final flow at the mid frame of (t, t+gap) against the known
motion; see opticalflowscivis_amd/flow_eval.py."""
from ..flow_eval import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 2)
