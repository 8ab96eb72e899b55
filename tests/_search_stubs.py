"""Stub predictors of the evolutionary search's fixtures: deterministic arithmetic on the arch dict, shared by
tests/golden/gen_golden_search.py (which runs the reference's EvolutionFinder with them) and tests/test_search_cpu.py (which
runs this library's).  TEST INFRASTRUCTURE."""

POPULATION_SIZE, MAX_TIME_BUDGET = 6, 3
CONSTRAINT = 2.0          # rejects the wide, high-resolution samples; the generator checks that every rejection loop ends
EVOLUTION_SEEDS = (3, 11)


def widths(arch):
    return [arch['input_channel']] + list(arch['deconv_setting']) + [s['channel'] for s in arch['backbone_setting']]


class StubEfficiency(object):
    """total channel count / 256, scaled by the resolution over 256"""

    def predict_eff(self, arch):
        return sum(widths(arch)) / 256.0 * (arch['img_size'] / 256.0)


class StubAccuracy(object):
    """A fixed polynomial of the widths and the resolution; ``calls`` keeps (accuracy, sample, efficiency) of every
    candidate in evaluation order."""
    COEF = (0.9, 0.31, 0.23, 0.17, 0.57, 0.41, 0.29, 0.13)

    def __init__(self):
        self.calls = []
        self._eff = StubEfficiency()

    def predict_acc(self, arch):
        w = widths(arch)
        acc = sum(c * v for c, v in zip(self.COEF, w)) / 100.0 - sum(v * v for v in w) / 40000.0 + arch['img_size'] / 2048.0
        self.calls.append((acc, arch, self._eff.predict_eff(arch)))
        return acc
