"""Sequence evaluation with the Flow-3D model (error.py:78-150, 374-436): `python -m opticalflowscivis_amd.flow3d.evaluate
--dataset jets3d --exp 1 2 3 --baseline --out result.json`; see opticalflowscivis_amd/evaluate.py."""
from ..evaluate import main
from .model.RIFE import Model

if __name__ == "__main__":
    main(Model, 3)
