"""Flow evaluation with the Flow-3D model: `python -m opticalflowscivis_amd.flow3d.evaluate_flow --dataset jets3d
--size 64 --gap 2 --zero-baseline --out result.json` scores the final flow at the mid frame of (t, t+gap) against the
known motion, converting the Flow-3D flow (rife3d convention) to a displacement; see opticalflowscivis_amd/flow_eval.py."""
from ..flow_eval import main_rife
from .model.RIFE import Model

if __name__ == "__main__":
    main_rife(Model, 3)
