// vo_odometry.cpp -- the reference's matching VO loop (VisualOdom::run, src/feature_matching.cpp:43-107) end to end
// on liborbx: images -> ORB -> 2-NN + ratio test -> get_pose -> get_scale -> pose chaining -> savePaths.
//
//   setup   : sorted frame list, readPoses, readCalib                          (:20-40, :126-153)
//   frame 0 : imread -> detectAndCompute; cur_pose = gt_pose                   (:54-57)
//   frame i : imread -> get_matches -> get_pose -> get_scale                   (:59-70)
//             T = [R | scale * t]; cur_pose = cur_pose * T.inv()               (:77-82)
//             kp1 = kp2; des1 = des2; prev_points_3d = points_3d               (:85-87)
//   end     : savePaths(gt_path.txt, est_path.txt, scale.txt)                  (:106)
// The reference draws the paths while it runs (drawPaths, cv::imshow); that is not reproduced.
//
// Usage: vo_odometry <kitti_dir> <seq> [max_frames] [nfeatures] [out_dir]
//   reads <kitti_dir>/data_odometry_gray/dataset/sequences/<seq>/{image_0/*.png, calib.txt} and
//   <kitti_dir>/data_odometry_poses/dataset/poses/<seq>.txt; writes the three files into out_dir (default: .)
//   and prints one line per frame: index, matches, estimated scale, true scale.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../visual-odometry-gpu_amd/host/kitti_io.hpp"
#include "../visual-odometry-gpu_amd/host/orb.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <kitti_dir> <seq> [max_frames] [nfeatures] [out_dir]\n", argv[0]);
    return 2;
  }
  try {
    const size_t max_frames = argc > 3 ? (size_t)std::atoi(argv[3]) : 1000;  // :51
    const int nfeatures = argc > 4 ? std::atoi(argv[4]) : 3000;              // cv::ORB::create(3000), :31
    const std::string out_dir = argc > 5 ? argv[5] : ".";
    const std::vector<std::string> images = orbx::io::list_sequence_images(argv[1], argv[2]);
    const std::vector<orbx::io::Mat4> gt_poses = orbx::io::read_poses(argv[1], argv[2]);
    const orbx::io::Mat3 K = orbx::io::read_calib(argv[1], argv[2]);
    auto orb = orbx::Feature2D::create(nfeatures);
    HammingMatcher matcher;
    std::vector<orbx::KeyPoint> kp1;
    orbx::DescriptorMat des1;
    orbx::VisualOdomState vo;
    std::vector<orbx::io::Point2d> gt_path, est_path;
    std::vector<double> gt_scale, est_scale;
    const auto t0 = std::chrono::high_resolution_clock::now();
    for (size_t i = 0; i < max_frames && i < images.size(); i++) {
      if (i >= gt_poses.size()) throw std::runtime_error("fewer ground-truth poses than frames");
      const orbx::io::Mat4& gt_pose = gt_poses[i];
      const orbx::io::GrayImage img = orbx::io::read_png_gray(images[i]);
      const orbx::Image view(img.pixels.data(), img.width, img.height);
      if (i == 0) {
        orb->detectAndCompute(view, kp1, des1);
        vo.cur_pose = gt_pose;
        std::printf("%zu %zu - -\n", i, kp1.size());
      } else {
        std::vector<orbx::KeyPoint> kp2;
        orbx::DescriptorMat des2;
        std::vector<orbx::Point2f> pts1, pts2;
        orbx::get_matches(*orb, matcher, kp1, des1, view, kp2, des2, pts1, pts2);
        double R[9], t[3];
        std::vector<uint8_t> mask;
        orbx::get_pose(pts1, pts2, K.data(), R, t, mask);
        std::vector<orbx::Point3f> points_3d;
        const double scale = orbx::get_scale(R, t, pts1, pts2, K.data(), points_3d, vo);
        const orbx::io::Mat4& prev = gt_poses[i - 1];
        const double dx = gt_pose[3] - prev[3], dy = gt_pose[7] - prev[7], dz = gt_pose[11] - prev[11];
        const double true_scale = std::sqrt(dx * dx + dy * dy + dz * dz);  // :72-73
        orbx::chain_pose(vo.cur_pose, R, t, scale);
        kp1 = kp2;
        des1 = des2;
        vo.shift(points_3d);
        gt_scale.push_back(true_scale);
        est_scale.push_back(scale);
        std::printf("%zu %zu %g %g\n", i, pts1.size(), scale, true_scale);
      }
      gt_path.push_back({gt_pose[3], gt_pose[11]});  // (x, z), :93-94
      est_path.push_back({vo.cur_pose[3], vo.cur_pose[11]});
    }
    const double sec = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    std::printf("elapsed %.3f s\n", sec);
    orbx::io::save_paths(out_dir + "/gt_path.txt", out_dir + "/est_path.txt", out_dir + "/scale.txt", gt_path, est_path,
                         gt_scale, est_scale);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
