"""The numpy restatement of the attention-dropout mask contract (tests/attention_dropout_cases.py): what makes the GPU comparison of
tests/test_attention_dropout_gpu.py mean something.  No GPU."""
import numpy as np

import attention_dropout_cases as ADC
import dropout_cases as DC

SEED, STEP, SITE = ADC.SEED, ADC.STEP, ADC.SITE0


def test_restatement_calls_the_pinned_philox():
    # (tests/test_dropout_cases_cpu.py checks dropout_cases.philox4x32_10 against the Random123 known answers)
    assert ADC.philox4x32_10 is DC.philox4x32_10 and ADC.threshold_of is DC.threshold_of and ADC.scale_of is DC.scale_of
    n, h, q, key, H = 3, 2, 5, 6, 3
    w = DC.philox4x32_10((n * H + h, (q << 16) | (key >> 2), SITE, STEP & 0xFFFFFFFF), (SEED & 0xFFFFFFFF, SEED >> 32))
    assert int(ADC.words(5, H, 7, SEED, STEP, SITE)[n, h, q, key]) == int(w[key & 3])


def test_mask_is_independent_of_N_and_K():
    small = ADC.words(5, 3, 7, SEED, STEP, SITE)
    big = ADC.words(9, 3, 40, SEED, STEP, SITE)
    assert np.array_equal(small, big[:5, :, :7, :7])
    for p in ADC.PS:
        assert np.array_equal(ADC.factors(5, 3, 7, p, SEED, STEP, SITE), ADC.factors(9, 3, 40, p, SEED, STEP, SITE)[:5, :, :7, :7])


def test_masks_differ_between_sites_steps_and_seeds():
    base = ADC.keep_mask(5, 3, 7, 0.5, SEED, STEP, SITE)
    for other in (ADC.keep_mask(5, 3, 7, 0.5, SEED, STEP, SITE + 1), ADC.keep_mask(5, 3, 7, 0.5, SEED, STEP + 1, SITE),
                  ADC.keep_mask(5, 3, 7, 0.5, SEED + 1, STEP, SITE), ADC.keep_mask(5, 3, 7, 0.5, SEED + (1 << 32), STEP, SITE)):
        # 735 fair coins: two independent masks agree on 367.5 +- 13.6 of them
        assert 250 < int((base == other).sum()) < 485
    # the attention sites are disjoint from the small ordinals of the feature-dropout sites
    assert SITE > 1 << 24


def test_tiny_p_has_threshold_zero_and_keeps_everything():
    assert DC.threshold_of(ADC.P_TINY) == 0
    assert bool(ADC.keep_mask(5, 3, 7, ADC.P_TINY, SEED, STEP, SITE).all())
    assert np.array_equal(ADC.factors(5, 3, 7, ADC.P_TINY, SEED, STEP, SITE), np.ones((5, 3, 7, 7), np.float32))


def test_kept_share_at_p_01():
    # binomial over 64 * 4 * 16 * 16 = 65 536 elements: sigma = sqrt(0.09 / 65 536) = 0.00117, 5 sigma = 0.006.
    # A condition on this fixed seed, not a measurement: the share is 0.901291 (59 067 of 65 536), 1.1 sigma above 0.9.
    share = float(ADC.keep_mask(64, 4, 16, 0.1, SEED, STEP, SITE).mean())
    assert abs(share - 0.9) <= 0.006
