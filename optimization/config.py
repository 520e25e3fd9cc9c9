"""``config.json`` of an optimisation folder as nested dictionaries whose keys are also attributes."""
import json


class Options(dict):
    """A dictionary whose items can also be read and set as attributes (``options.mesh.tiling``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value

    def __delattr__(self, name):
        del self[name]


def wrap(value):
    """Dictionaries anywhere inside `value` (also inside lists) become Options; everything else is returned as it is."""
    if isinstance(value, dict):
        return Options((k, wrap(v)) for k, v in value.items())
    if isinstance(value, list):
        return [wrap(v) for v in value]
    return value


def load_json(path):
    with open(path) as fh:
        return wrap(json.load(fh))
