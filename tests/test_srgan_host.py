"""The standard-GAN step's host side (no GPU): the exported entry and its argument check, the ``gan_type`` names, the
update schedule of ``train.SRGANStep``, and what it refuses or accepts before any launch."""
import pytest
import torch


def test_gan_loss_entry_is_exported_and_checks_its_arguments():
    import ctypes as C
    from esrganplus_amd import _lib as L
    assert 'esr_gan_loss_forward' in L.EXPORTS
    so = C.CDLL(L.LIB_PATH)
    assert hasattr(so, 'esr_gan_loss_forward')
    lib = L.lib()
    assert lib.esr_gan_loss_forward(None, None) == -1
    assert b'esr_gan_loss_forward' in lib.esr_last_error()
    assert lib.esr_abi_version() == 6


def test_gan_type_names():
    from esrganplus_amd import losses as LS
    with pytest.raises(NotImplementedError, match='double backward'):
        LS.GANLoss('wgan-gp')
    with pytest.raises(NotImplementedError, match=r'GAN type \[foo\] is not found'):
        LS.GANLoss('foo')
    assert LS.GANLoss('LSGAN').gan_type == 'lsgan' and LS.GANLoss('Vanilla', 0.9, 0.1).real_label_val == 0.9
    assert LS.gan_kind('vanilla') == 0 and LS.gan_kind('lsgan') == 1


@pytest.mark.parametrize('ratio,init,moves', [(1, 0, [1, 2, 3, 4, 5, 6]), (2, 1, [2, 4, 6]), (3, 0, [3, 6])])
def test_generator_update_schedule(ratio, init, moves):
    """SRGAN_model.py:119: ``step % D_update_ratio == 0 and step > D_init_iters`` over iterations 1..6."""
    from esrganplus_amd import train
    assert [it for it in range(1, 7) if train.SRGANStep.g_update_due(it, ratio, init)] == moves


def _cpu_nets():
    from esrganplus_amd import architecture as arch
    return arch.RRDBNet(3, 3, 64, 1), arch.Discriminator_VGG_128(3, 64)


def test_step_refuses_cpu_tensors_and_builds_without_netF():
    from esrganplus_amd import train, _lib as L
    netG, netD = _cpu_nets()
    st = train.SRGANStep(netG, netD, None, pixel_weight=0, feature_weight=0, data_parallel=False)
    assert st.netF is None and st.l_fea_w == 0 and st.l_pix_w == 0 and st.iteration == 0
    with pytest.raises(L.HipExtensionError, match='SRGANStep.step: var_L'):
        st.step(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        train.SRGANStep(netG, netD, None, data_parallel=False)                      # a feature term without netF
    with pytest.raises(NotImplementedError):
        train.SRGANStep(netG, netD, None, feature_weight=0, gan_type='wgan-gp', data_parallel=False)
    st2 = train.SRGANStep(netG, netD, None, feature_weight=0, gan_type='LSGAN', D_update_ratio=None, D_init_iters=None,
                          data_parallel=False)
    assert st2.gan_type == 'lsgan' and (st2.D_update_ratio, st2.D_init_iters) == (1, 0)
    assert set(st2.state_dict()) == {'optimizers', 'iter'}
