"""STN factory and command-line flags of the registration network: the drop-in contract of reference models/stn/__init__.py
(flag names and defaults :10-25, `define_stn(opt, stn_type)` :28-48).  Names / types / defaults are the interface and are identical;
everything else is this build's own."""
from .affine_stn import AffineSTN
from .unet_stn import UnetSTN

sampling_align_corners = False
sampling_mode = 'bilinear'

# (flag, argparse keywords, train-only) — the reference's five --stn_* options
_FLAGS = (
    ('--stn_cfg', dict(type=str, default='A',
                       help="layer table of the registration net: 'A' (the reference's), 'deep' (9 levels, for 1024x1024 inputs)"), False),
    ('--stn_type', dict(type=str, default='affine',
                        help='registration model: affine (6 parameters per pair) | unet (dense deformation field)'), False),
    ('--stn_bilateral_alpha', dict(type=float, default=0.0,
                                   help='unet only: edge-aware weight exp(-alpha |dI|) on the smoothness penalty; 0 switches it off'), True),
    ('--stn_no_identity_init', dict(action='store_true',
                                    help='unet only: start from a random field instead of the near-identity initialisation'), True),
    ('--stn_multires_reg', dict(type=int, default=1,
                                help='unet only: apply the smoothness penalty at this many resolutions (1 = full resolution only)'), True),
)


def _integrate(opt):
    """--stn_integrate (0 where the option set does not carry it: a Namespace built before the flag existed)"""
    return int(getattr(opt, 'stn_integrate', 0))


def _flag(opt, name):
    """opt.<name>, or the flag's default where the command line did not carry it (the train-only flags on a test command line: they
    configure the regulariser and the initialisation, which inference does not use)"""
    kw = next(kw for flag, kw, _ in _FLAGS if flag == '--' + name)
    return getattr(opt, name, kw.get('default', False))


_BUILDERS = {
    'affine': lambda a, b, h, w, opt: AffineSTN(a, b, h, w, opt.stn_cfg, opt.init_type),
    'unet': lambda a, b, h, w, opt: UnetSTN(a, b, h, w, opt.stn_cfg, opt.init_type, _flag(opt, 'stn_bilateral_alpha'),
                                            not _flag(opt, 'stn_no_identity_init'), _flag(opt, 'stn_multires_reg'),
                                            integrate=_integrate(opt)),
}


def modify_commandline_options(parser, is_train=True):
    import argparse
    for flag, kw, train_only in _FLAGS:
        if is_train or not train_only:
            parser.add_argument(flag, **kw)
    # (MI355X build) diffeomorphic UNet STN: the network's output as a stationary velocity field, the warp reads exp(v) integrated by K
    # scaling-and-squaring steps (ops.integrate_velocity).  For train AND test: a checkpoint trained with it must be registered with it.
    # SUPPRESS: an option set without the flag is the set of before it existed (read with getattr(opt, 'stn_integrate', 0))
    parser.add_argument('--stn_integrate', type=int, default=argparse.SUPPRESS,
                        help='unet only: integrate the predicted field as a stationary velocity by this many scaling-and-squaring steps '
                             '(0 = off: the field is the displacement, as the reference has it; 6 is a usual choice)')
    return parser


def define_stn(opt, stn_type='affine'):
    """The STN for `opt`, on this process's GPU.  One process drives one GPU (no nn.DataParallel wrap, hence no `.module`
    indirection); an unknown type gives None, as the reference's factory does."""
    import torch
    make = _BUILDERS.get(stn_type)
    if make is None:
        return None
    k = _integrate(opt)
    if k < 0 or k > 30:
        raise ValueError('--stn_integrate %d: the number of squaring steps, 0 .. 30' % k)
    if k > 0 and stn_type != 'unet':
        raise ValueError('--stn_integrate %d needs --stn_type unet: the %s STN predicts no field to integrate' % (k, stn_type))
    a_to_b = opt.direction == 'AtoB'
    net = make(opt.input_nc if a_to_b else opt.output_nc, opt.output_nc if a_to_b else opt.input_nc, opt.img_height, opt.img_width, opt)
    if len(opt.gpu_ids) > 0:
        assert torch.cuda.is_available()
        net.to(torch.device('cuda', opt.gpu_ids[0]))
    return net
