"""examples/config.py: the yaml as a nested attribute object.

The reference's `Config` spells its constructor `init` (examples/config.py:7), so `Config(hps)` raises a TypeError there and
`load_config` cannot return.  That bug is not kept: this `Config` has a working `__init__` and otherwise the same behaviour (dicts
become Config objects, also inside lists and tuples; everything else is kept as it is)."""
from pprint import pformat

import yaml


class Config:
    def __init__(self, cfg_dict):
        for k, v in cfg_dict.items():
            if isinstance(v, (list, tuple)):
                setattr(self, k, [Config(x) if isinstance(x, dict) else x for x in v])
            else:
                setattr(self, k, Config(v) if isinstance(v, dict) else v)

    def __str__(self):
        return pformat(self.__dict__)

    def __repr__(self):
        return self.__str__()


def load_config(path):
    with open(path) as stream:
        return Config(yaml.load(stream, yaml.SafeLoader))
