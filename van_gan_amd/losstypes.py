"""The selectable loss types of the reference's loss functions (pure host logic, no GPU): ``cycle_loss(typ=None | "mse" | "L4" | "bce")``
(loss_functions.py:163-190) and ``generator_loss_fn`` / ``discriminator_loss_fn(typ=None | "bce" | "bfce", from_logits=True)``
(:255-322).  The reference's VanGan hard-codes one choice at its call sites (vangan.py:302,306,329-332): 'bce' for the S -> I -> S
cycle, 'mse' for the I -> S -> I cycle, LSGAN for the adversarial terms -- the engine's defaults."""
from __future__ import annotations

from typing import Optional, Tuple

CYCLE_LOSSES = ('mae', 'mse', 'L4', 'bce')          # 'mae' is the reference's typ=None (its own default: the CycleGAN L1 term)
GAN_LOSSES = (None, 'bce', 'bfce')                  # None is LSGAN
LP_ORDER = {'mae': 1, 'mse': 2, 'L4': 4}            # p of vg_lp_loss


def check_loss_types(cycle_loss_SIS='bce', cycle_loss_ISI='mse', gan_loss=None, wasserstein: bool = False) -> Tuple[str, str, Optional[str]]:
    """Raise ValueError for anything but the listed names.  (The reference falls through to its last branch for every cycle type it
    does not know and silently trains the BCE term; an unknown adversarial type fails later on an unbound name.  Neither is copied.)"""
    for arg, v in (('cycle_loss_SIS', cycle_loss_SIS), ('cycle_loss_ISI', cycle_loss_ISI)):
        if not isinstance(v, str) or v not in CYCLE_LOSSES:
            raise ValueError("%s must be one of 'mae' (the reference's typ=None), 'mse', 'L4', 'bce', got %r (the reference silently treats "
                             "every unknown string as 'bce', loss_functions.py:185-190; this engine does not)" % (arg, v))
    if gan_loss is not None and (not isinstance(gan_loss, str) or gan_loss not in GAN_LOSSES):
        raise ValueError("gan_loss must be None (LSGAN), 'bce' or 'bfce', got %r (the reference binds no loss object for any other "
                         "string and fails on the unbound name, loss_functions.py:275-285; this engine raises here)" % (gan_loss,))
    if gan_loss is not None and wasserstein:
        raise ValueError('gan_loss=%r with wasserstein=True: the Wasserstein branch never calls generator_loss_fn / discriminator_loss_fn '
                         '(vangan.py:322-326)' % (gan_loss,))
    return cycle_loss_SIS, cycle_loss_ISI, gan_loss
