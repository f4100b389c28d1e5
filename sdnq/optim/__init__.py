"""sdnq.optim of the import-name drop-in: the optimizers of ``sdnq_amd.optim`` at the reference's module paths (``sdnq.optim``,
``.adamw``, ``.optimizer``, ``.utils``); no arithmetic lives here.  ``AdamW`` is built; ``Adafactor``, ``CAME``, ``Lion`` and ``Muon``
import and raise NotImplementedError naming themselves."""
from sdnq_amd.optim import CAME, Adafactor, AdamW, Lion, Muon, SDNQOptimizer  # noqa: F401

__all__ = ["SDNQOptimizer", "Adafactor", "AdamW", "CAME", "Lion", "Muon"]
