"""hifi_gan/env.py: the attribute-access dict the HiFi-GAN config json is read into."""
from __future__ import annotations


class AttrDict(dict):
    """A dict whose keys are also attributes (``h.upsample_rates``), as the reference's env.py:5-8."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self
