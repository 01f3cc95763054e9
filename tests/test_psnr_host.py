"""Host side of the PSNR-oriented pretraining step (train.PSNRStep) and the l2 criterion: the library exports the new
entry under the unchanged ABI, the criterion names are the reference's, and nothing runs without a GPU."""
import ctypes as C

import pytest
import torch


def test_library_exports_the_l2_entry_under_abi_6():
    from esrganplus_amd import _lib as L
    assert 'esr_l2_loss_forward' in L.EXPORTS
    lib = L.lib()                                             # loads the library: every exported symbol present
    assert hasattr(C.CDLL(L.LIB_PATH), 'esr_l2_loss_forward')
    assert lib.esr_abi_version() == 6
    assert lib.esr_l2_loss_forward.argtypes[0] == C.POINTER(L.esr_l1_loss)      # the l1 argument struct, unchanged
    assert lib.esr_l2_loss_forward(None, None) == -1                            # ESR_ERR_INVALID, before any launch
    assert b'esr_l2_loss_forward' in lib.esr_last_error()
    assert lib.esr_l1_loss_forward(None, None) == -1
    assert b'esr_l1_loss_forward' in lib.esr_last_error()


def test_unknown_criteria_are_refused_with_the_references_message():
    from esrganplus_amd import architecture as arch, train, losses as LS
    netG = arch.RRDBNet(3, 3, 64, 1)
    with pytest.raises(NotImplementedError, match=r'^Loss type \[l3\] is not recognized\.$'):
        train.PSNRStep(netG, pixel_criterion='l3')
    for kw in ({'pixel_criterion': 'l3'}, {'feature_criterion': 'l3'}):
        with pytest.raises(NotImplementedError, match=r'^Loss type \[l3\] is not recognized\.$'):
            train.ESRGANPlusStep(netG, None, None, **kw)
    assert LS.criterion('l1') == (LS.l1_raw, LS.l1_loss) and LS.criterion('l2') == (LS.l2_raw, LS.l2_loss)


def test_psnr_step_has_no_cpu_path():
    from esrganplus_amd import architecture as arch, train, losses as LS, _lib as L
    netG = arch.RRDBNet(3, 3, 64, 1).train()
    st = train.PSNRStep(netG, pixel_criterion='l2', weight_decay_G=1e-2)
    assert st.optimizer_G.param_groups[0]['lr'] == 2e-4 and st.optimizer_G.param_groups[0]['weight_decay'] == 1e-2
    assert isinstance(st.optimizer_G, torch.optim.Optimizer) and st.scaler is None and not st.exG.enabled
    lr, hr = torch.rand(1, 3, 8, 8), torch.rand(1, 3, 32, 32)
    with pytest.raises(L.HipExtensionError):
        st.step(lr, hr)
    with pytest.raises(L.HipExtensionError):
        st.test(lr)
    assert netG.training
    with pytest.raises(L.HipExtensionError):
        LS.l2_raw(lr, lr, 1.0)
    with pytest.raises(L.HipExtensionError):
        LS.l2_loss(lr, lr)
