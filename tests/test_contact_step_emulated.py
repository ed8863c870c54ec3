"""Emulated twin of tests/test_gpu_contact_step.py (tests/contact_step_cases.py): the product's kernels on the CPU emulator -- and, what
only the emulator can do, the planted batch under the identity and the reverse wavefront order (tests/test_wave_order.py): a hand-over
between wavefront 0 and its helper that no barrier orders would change the bits.  At the emulator's sizes (CC.EMULATED: 7 envs against
the device's 13); the batch in which every env gives up is tests/test_schedule_emulated.py's."""
import contact_step_cases as CC
from test_wave_order import PAIR, Waves


def test_emulated_shipped_contact_step_is_the_other_kernels_step_bit_for_bit(emu_library):
    CC.check_shipped_schedule(library=emu_library, case=CC.EMULATED)


def test_emulated_contact_step_under_either_wavefront_order(emu_library):
    waves = Waves(emu_library)
    c = CC.EMULATED
    st, a = CC.batch(c['N'], c['pressed'], c['prone'], c['given_up'])
    base = CC.step_once(emu_library, st, a)
    CC.check_lists(base, c['N'], c['pressed'], c['prone'], c['given_up'], 'default scheduler')
    for order in PAIR:
        before = waves.launches()
        with waves.order(order):
            got = CC.step_once(emu_library, st, a)
        assert waves.launches() > before, order            # the two-wavefront workgroups did run under the list
        CC.same_bits(got, base, 'wavefront order %s against the default scheduler' % (order,))
        assert sorted(got['sched']['redo'].tolist()) == c['given_up']


def test_emulated_every_live_wavefront_leaves_one_trace_record(emu_library):
    CC.check_trace(library=emu_library, case=CC.EMULATED)
