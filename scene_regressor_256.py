"""reference scene_regressor_256.py — training the 40-attribute ResNet-50 regressor (MI355X-native: latent2im_amd/regressor_train.py)."""
from latent2im_amd.regressor_train import (CustomDataset, TrainableResNet50, load_ckpt, load_labelfile, main, make_optimizer,  # noqa: F401
                                           save_ckpt, train_step)


def parse_args(argv=None):
    """No flag: the reference's run, as before.  The flags only name what main() takes."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--image_size', type=int)
    ap.add_argument('--n_epoch', type=int)
    ap.add_argument('--batch_size', type=int)
    ap.add_argument('--out_dir')
    ap.add_argument('--resident', action='store_true', help='resident model: gradient arena, in-place weight repack, BatchNorm algebra and Adam on the device')
    ap.add_argument('--hip_graph', action='store_true', help='replay every full batch from one hipGraph (implies --resident)')
    ap.add_argument('--device_data', action='store_true', help='decode the training split once and keep it on the GPU as uint8')
    ap.add_argument('--precision', choices=('f32', 'f16', 'bf16'), help='f16 / bf16: h8 maps and the 16-bit MFMA (fp32 master weights, implies --resident); '
                                                                        'f16 is the recommended 16-bit type')
    ap.add_argument('--loss_scale_log2', type=int, help='static loss-scale exponent of the 16-bit path (default: regtrain_scale_for for f16, 0 for bf16)')
    return {k: v for k, v in vars(ap.parse_args(argv)).items() if v is not None and v is not False}


if __name__ == '__main__':
    main(**parse_args())
