from . import inference, group, loss, trainer  # noqa: F401
