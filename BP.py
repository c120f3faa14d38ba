"""Drop-in for the reference's ``BP.py`` (inversion of real images into W+), same flags:

python BP.py --batch_size 1 --optimizer Adam --dataset ffhq --n_loops 4000 --path ./data/face --save_path ./results_face \
        [--resolution 256 --lr 0.01 --synthetic_weights]

``--path`` is an image folder with class sub-folders; ``--save_path`` receives org_i.png, i_final.png, latent/i_w.npy and loss_back.npy.
The saved latents feed ``vis_w.py --given_w``.
"""
from latent2im_amd.bp import main

if __name__ == '__main__':
    main()
